"""Device tests of the inverse transform (``csrc/pdehip_fft.hip``) and of the direct Poisson solve (``csrc/pdehip_fftsolve.hip``):
``pdehip_fft_inverse`` and ``pdehip_poisson_fft`` through the C ABI against the serial C versions of the tests-only shim - EQUAL BITS of
every output element - and ``method="fft"`` of the ``poisson_solver`` operator.

Inputs, drivers, bounds and the shim's results (computed once per case): ``tests/poisson_fft_cases.py``.  The shim itself is checked
against numpy, the dense restatement and the reference's golden solutions in ``tests/test_poisson_fft_cpu.py``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import poisson_fft_cases as P
import pytest
import spectrum_cases as K
from helpers import GOLDEN, get_case, load_cases, make_grid

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray, DeviceBuffer, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

IDS = ["f64", "f32"]
NPZ = np.load(GOLDEN / "poisson_fft.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def lib():
    return pde_hip.get_backend("hip")._lib


# ---- the inverse transform ---------------------------------------------------------------------------------------------------------------
def check_inverse(lib, shape, ncomp, dtype):
    name = np.dtype(dtype).name
    spec = K.shim_forward(shape, ncomp, "float64")
    got, before, after = P.fft_inverse(lib, shape, spec, dtype)
    expect = P.shim_inverse(shape, ncomp, name)
    differ = np.count_nonzero(P.bits(got) != P.bits(expect))
    print(f"{K.shape_id(shape)} c{ncomp} {name}: {differ} of {got.size} words differ; {lib.last_kernel_name().decode()}")
    assert got.shape == expect.shape and got.dtype == expect.dtype and differ == 0
    # the whole output allocation: what is not an interior cell equals the uploaded pattern, word for word
    outside = ~P.interior_mask(lib, DeviceArray(GridInfo(shape, (1.0,) * len(shape), np.dtype(dtype)), (ncomp,)))
    assert outside.any()
    np.testing.assert_array_equal(after[outside], before[outside], err_msg="ghost cells, row padding or slack were written")
    chain = lib.last_kernel_name().decode().split("+")
    assert chain[-1] == f"inverse_rows_kernel<{'double' if name == 'float64' else 'float'}>"
    assert chain[:-1] == ["inverse_lines_kernel"] * sum(n > 1 for n in shape[:-1])


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("ncomp", K.NCOMPS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_fft_inverse_equals_the_shim(lib, shape, ncomp, dtype):
    check_inverse(lib, shape, ncomp, dtype)


def test_fft_inverse_beyond_the_turn(lib):
    check_inverse(lib, K.TURN, 3, np.float64)


def test_forward_names_are_unchanged(lib):
    shape = (2, 64, 8)
    dev = K.upload(lib, shape, K.inputs(shape, 1, "float64"))
    K.fft_forward(lib, dev)
    assert lib.last_kernel_name().decode() == "fft_rows_kernel<double>+fft_lines_kernel+fft_lines_kernel"


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------
def check_solve(lib, shape, dtype):
    name = np.dtype(dtype).name
    rhs = P.solve_input(shape, name)
    dx = K.dx_of(shape)
    got, io, chain = P.poisson_fft(lib, shape, dx, rhs)
    expect, e_io = P.shim_solve(shape, name)
    differ = np.count_nonzero(P.bits(got) != P.bits(expect))
    print(f"{K.shape_id(shape)} {name}: {differ} of {got.size} words differ; {io}; {chain}")
    assert got.dtype == expect.dtype and differ == 0
    P.check_io(io, e_io, P.cells_of(shape))
    assert chain == P.expected_chain(shape, dtype)
    again, io2, _ = P.poisson_fft(lib, shape, dx, rhs)
    np.testing.assert_array_equal(P.bits(again), P.bits(got), err_msg="two calls differ")
    assert io2 == io


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_poisson_fft_equals_the_shim(lib, shape, dtype):
    check_solve(lib, shape, dtype)


def test_poisson_fft_beyond_the_turn(lib):
    check_solve(lib, K.TURN, np.float64)


def test_inconsistent_and_nonfinite_right_hand_sides(lib):
    """The violating-cell decision and the status are the shim's."""
    shape, dx = (16, 8), (0.75, 1.5)
    holed = P.white(shape)
    holed[3, 3] = np.nan
    for rhs in (P.white(shape, mean=1.0), P.white(shape, mean=1e-4), holed):
        got, io, _ = P.poisson_fft(lib, shape, dx, rhs)
        expect, e_io = P.shim().solve(shape, dx, rhs)
        assert io["status"] == e_io["status"] and io["status"] in (2, 4)
        if io["status"] == 4:
            np.testing.assert_array_equal(P.bits(got), P.bits(expect))
            P.check_io(io, e_io, P.cells_of(shape))
    got, io, _ = P.poisson_fft(lib, shape, dx, P.white(shape), rtol=0.0, atol=0.0)
    assert io["status"] == 1
    assert P.poisson_fft(lib, shape, dx, P.white(shape), rtol=0.0, atol=1e-9)[1]["status"] == 0


def test_release_scratch(lib):
    shape = (16, 4, 128)
    rhs, dx = P.solve_input(shape, "float64"), K.dx_of(shape)
    before = P.poisson_fft(lib, shape, dx, rhs)
    lib.release_scratch()
    after = P.poisson_fft(lib, shape, dx, rhs)
    np.testing.assert_array_equal(P.bits(before[0]), P.bits(after[0]))
    assert before[1] == after[1]
    np.testing.assert_array_equal(P.bits(after[0]), P.bits(P.shim_solve(shape, "float64")[0]))


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
def test_two_streams(lib, dtype):
    """Two streams solve on two grids of different shapes and spacings: each gets the result it gets alone (spectrum, tables, work arrays
    and slots are kept per stream).  Both wait for an event behind a queue of copies on a third stream, as in
    test_hip_spectrum.py::test_two_streams."""
    name = np.dtype(dtype).name
    shapes = [(8, 8, 256), (16, 4, 128)]
    alone = [P.shim_solve(s, name) for s in shapes]
    big = GridInfo((65, 129, 251), (1.0,) * 3, np.float64)
    src, copy = DeviceArray(big, (1,)), DeviceArray(big, (1,))
    lib.memset(src.ptr, 0, src.nbytes, None)
    one, table = (C.c_double * 1)(1.0), ptr_array([src])
    streams, event = [], C.c_void_p()
    for _ in range(3):
        s = C.c_void_p()
        lib.stream_create(C.byref(s))
        streams.append(s)
    lib.event_create(C.byref(event))
    try:
        for _ in range(100):
            lib.lincomb(big.ref, 1, copy.ptr, None, 1, one, table, streams[2])
        lib.event_record(event, streams[2])
        for q in range(2):
            lib.stream_wait_event(streams[q], event)
        for q in (0, 1, 0, 1):
            got, io, _ = P.poisson_fft(lib, shapes[q], K.dx_of(shapes[q]), P.solve_input(shapes[q], name), stream=streams[q])
            np.testing.assert_array_equal(P.bits(got), P.bits(alone[q][0]), err_msg=f"stream {q}")
            P.check_io(io, alone[q][1], P.cells_of(shapes[q]))
    finally:
        for s in streams:
            lib.stream_synchronize(s)
            lib.stream_destroy(s)
        lib.event_destroy(event)


def test_refusals(lib):
    shape = (4, 8)
    dev = K.upload(lib, shape, K.inputs(shape, 1, "float64"))
    out = K.upload(lib, shape, K.inputs(shape, 1, "float64"))
    ref = dev.info.ref
    spec = DeviceBuffer(4096)
    lib.memset(spec.ptr, 0, spec.nbytes, None)
    io = _abi.Poisson()
    io.rtol, io.atol = 1e-10, 0.0
    lib.fft_inverse(ref, 1, spec.ptr, out.ptr, None)
    lib.poisson_fft(ref, dev.ptr, out.ptr, C.byref(io), None)
    for args in ((ref, 1, None, out.ptr), (ref, 1, spec.ptr, None), (ref, 0, spec.ptr, out.ptr), (ref, 65, spec.ptr, out.ptr),
                 (ref, 1, spec.ptr + 8, out.ptr), (ref, 1, spec.ptr, out.ptr + 8)):
        with pytest.raises(ValueError):
            lib.fft_inverse(*args, None)
    for args in ((ref, None, out.ptr, C.byref(io)), (ref, dev.ptr, None, C.byref(io)), (ref, dev.ptr, out.ptr, None),
                 (ref, dev.ptr + 8, out.ptr, C.byref(io)), (ref, dev.ptr, out.ptr + 8, C.byref(io))):
        with pytest.raises(ValueError):
            lib.poisson_fft(*args, None)
    bad = _abi.Poisson()
    bad.rtol, bad.atol = -1.0, 0.0
    with pytest.raises(ValueError):
        lib.poisson_fft(ref, dev.ptr, out.ptr, C.byref(bad), None)
    for shape in K.REFUSED:
        info = GridInfo(shape, (1.0,) * len(shape), np.float64)
        with pytest.raises(NotImplementedError, match="axis"):
            lib.fft_inverse(info.ref, 1, spec.ptr, out.ptr, None)
        with pytest.raises(NotImplementedError, match="axis"):
            lib.poisson_fft(info.ref, dev.ptr, out.ptr, C.byref(io), None)
    grid = pde_hip.UnitGrid([8, 8], periodic=[True, False])
    with pytest.raises(NotImplementedError, match="lower face of axis 1"):
        grid.make_operator("poisson_solver", ["periodic", {"value": 0}], backend="hip", method="fft")
    with pytest.raises(NotImplementedError, match="axis"):
        pde_hip.UnitGrid([12, 8], periodic=True).make_operator("poisson_solver", "periodic", backend="hip", method="fft")


# ---- through the operator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in load_cases(NPZ) if not c.get("raises")])
def test_golden_solutions(cid):
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    op = grid.make_operator("poisson_solver", case["bc"], backend="hip", method="fft")
    got, want = op(NPZ[f"{cid}/rhs"]), NPZ[f"{cid}/solution"]
    assert abs(got.mean()) < 1e-10
    want = want - want.mean()
    assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) < 1e-8
    assert op.info["method"] == "fft" and op.info["iterations"] == 0 and op.info["converged"]
    assert op.info["residual"] <= 1e-11 * op.info["rhs_norm"]
    assert pde_hip.get_backend("hip")._lib.last_kernel_name().decode().endswith("+fftsolve_check_kernel")
    res = pde_hip.solve_poisson_equation(pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"]), case["bc"], method="fft")
    assert res.label == str(NPZ[f"{cid}/label"]) and np.array_equal(res.data, got)


def test_inconsistent_right_hand_side_raises_like_the_reference():
    (cid,) = [c["id"] for c in load_cases(NPZ) if c.get("raises")]
    case = get_case(NPZ, cid)
    grid = make_grid(case)
    rhs = pde_hip.ScalarField(grid, NPZ[f"{cid}/rhs"])
    with pytest.raises(RuntimeError) as err:
        pde_hip.solve_poisson_equation(rhs, case["bc"], method="fft")
    want = str(NPZ[f"{cid}/message"])
    assert str(err.value).split("magnitude")[0] == want.split("magnitude")[0]
    assert "Poisson problem could not be solved (Residual:" in str(err.value.__cause__)


def test_a_resident_right_hand_side_is_solved_without_a_transfer():
    """A 32^3 diffusion run; the callback solves Poisson's equation for the resident state between the stepper calls: the state stays on
    the device (the transfer counter the spectrum tests use) and the answer is that of the operator on a side copy."""
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([32, 32, 32], periodic=True)
    state = pde_hip.ScalarField(grid, K.cosine_field((32, 32, 32), ((2, (0, 3, 0)), (1, (4, 0, 1)))))
    op = grid.make_operator("poisson_solver", "periodic", backend=backend, method="fft")
    seen = []

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        if link is None or not link.host_stale:
            return
        res = op(link.dev_state)
        assert isinstance(res, DeviceArray) and link.downloads == 0 and link.host_stale
        exact = link.dev_state.get_valid()          # a side copy for the reference: not a download of the field
        np.testing.assert_array_equal(res.get_valid(), op(exact))
        seen.append(t)

    res = pde_hip.DiffusionPDE(1.0).solve(state, t_range=2.0, dt=0.1, solver="euler", backend=backend, tracker=callback, interval=0.5)
    assert len(seen) >= 3 and res.__dict__["_hip_link"].downloads == 0


def test_fft_and_mgcg_agree():
    """A sanity link between the two solvers at 64^3, not the accuracy claim."""
    shape = (64, 64, 64)
    grid = pde_hip.UnitGrid(list(shape), periodic=True)
    rhs = P.white(shape)
    direct = grid.make_operator("poisson_solver", "periodic", backend="hip", method="fft")
    mg = grid.make_operator("poisson_solver", "periodic", backend="hip", method="mgcg", rtol=1e-12)
    a, b = direct(rhs), mg(rhs)
    print(f"max |fft - mgcg| = {np.abs(a - b).max():.3g}, max |x| = {np.abs(a).max():.3g}; {direct.info}; {mg.info}")
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
