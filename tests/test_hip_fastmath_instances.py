"""The contracted build (`pdehip_set_fastmath`, namespace ``pdehip::fastv``) instance by instance: every case of tests/fastmath_cases.py goes through
the C ABI / the host mirror exactly as the exact-build test it was drawn from, once per arithmetic mode.

Default mode: the oracle's bits (the wiring of the case).  ``backend.fastmath = True``: the same kernel instance of the other build
(`pdehip_last_kernel_name`), a finite result, and ``|result - reference| <= bound`` in every cell, where reference and bound are the running-error
evaluation of the oracle's own expression (tests/fastmath_cases.py; tied to the oracle and to a contracted CPU build by
tests/test_fastmath_cases_cpu.py) - no tolerance is chosen by hand.  Cases whose expression has no product feeding a sum must keep the oracle's bits.
Afterwards the default mode gives the oracle's bits again.

Not covered here: the generic kernels behind PDEHIP_FORCE_GENERIC (read once per process), the decomposed (slab / block) loops, and the pure-fp32
mode (it has no contracted twin).  tests/test_hip_fastmath.py keeps its whole solves of 200 steps.
"""

from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest
from fastmath_cases import CASES, FAMILIES, IDS, OPERATORS, SINGLE_BUILD, Built, Case, bounds_of, build_case, excess, worst_ratio

import pde_hip
from pde_hip import _abi
from pde_hip.backend import convert_bcs
from pde_hip.device import DeviceArray, DeviceBuffer, DeviceScalar, GridInfo, ptr_array

pytestmark = pytest.mark.gpu

# what the run reached, for the summary of a change to these kernels: printed when the module is done (pytest -s)
REPORT: dict[str, dict] = {}


@pytest.fixture
def backend():
    b = pde_hip.get_backend("hip")
    yield b
    b.fastmath = None
    _ = b._lib   # applies the default mode again


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if not REPORT:
        return
    # (fp32 storage: the rounding to fp32 alone takes up to the whole bound of a cell, so that figure sits just below 1 by construction)
    out = {fam: {"cases": r["cases"], "worst |result - reference| / bound": r["ratio"], "cases with other bits than the oracle": r["differs"],
                 "instances": sorted(r["names"])} for fam, r in REPORT.items()}
    text = json.dumps(out, indent=1)
    print("\ncontracted build, per launch family:\n" + text)


# ---------------------------------------------------------------------------------------------------------------------------------
# the name of the instance a call launched.  Not every kernel records one (the ghost-cell and one-cell-per-thread kernels do
# not), and the library keeps the last name: a three-step launch of the 2-D tile kernel - a step count no case uses - marks the spot,
# and a name equal to the mark afterwards means that the call recorded none.
# ---------------------------------------------------------------------------------------------------------------------------------
_MARK = {}


def _mark(backend):
    if not _MARK:
        grid = pde_hip.UnitGrid([5, 7], periodic=True)
        data = np.zeros(grid.shape)
        spec = backend.make_rhs_spec(pde_hip.DiffusionPDE(0.5), pde_hip.ScalarField(grid, data))
        _MARK.update(spec=spec, a=DeviceArray(spec.info).set_valid(data), b=DeviceArray(spec.info))
    lib, done = backend._lib, C.c_int(0)
    lib.euler_multi_2d(_MARK["spec"].info.ref, _MARK["spec"].ref, _MARK["a"].ptr, _MARK["b"].ptr, 0.01, 3, C.byref(done), None)
    assert done.value == 1
    name = lib.last_kernel_name().decode()
    assert "(3 steps per launch" in name, name
    return name


def _name_since(backend, mark):
    name = backend._lib.last_kernel_name().decode()
    return "" if name == mark else name


def _must_record_a_name(case: Case):
    if case.opt("instance") or case.family in ("launch_euler2", "launch_euler4", "launch_tile2d"):
        return True
    # the vectorised Laplacian / gradient kernel: two axes or more and rows aligned on both sides (full output)
    return case.family in ("launch_laplace", "launch_deriv_march") and len(case.shape) >= 2 and case.opt("layout", "full") == "full"


# ---------------------------------------------------------------------------------------------------------------------------------
# one call (or one short run) of a case on the device: ([results], done flag or None)
# ---------------------------------------------------------------------------------------------------------------------------------
def _device_run(backend, built: Built):
    c, grid, dtype, data = built.case, built.grid, built.dtype, built.data
    lib, e, nd = backend._lib, built.case.entry, len(built.case.shape)
    if e == "set_ghost_cells" or e in OPERATORS:
        info = backend.grid_info(grid, dtype)
        dev = DeviceArray(info, (nd,) * built.rank).set_valid(data)
        backend.make_ghost_cell_setter(built.bcs_c)(dev)
        if e == "set_ghost_cells":
            return [dev.get_hostfull()], None
        layout = _abi.OUT_FULL if c.opt("layout", "full") == "full" else _abi.OUT_VALID
        ncomp_out = nd if e == "gradient" else 1

        def run(call):
            if layout == _abi.OUT_FULL:
                out = DeviceArray(info, (ncomp_out,) if ncomp_out > 1 else ())
                call(out.ptr)
                return out.get_valid()
            buf = DeviceBuffer(c.cells * ncomp_out * dtype.itemsize)
            call(buf.ptr)
            host = np.empty(((ncomp_out,) if ncomp_out > 1 else ()) + tuple(c.shape), dtype)
            lib.memcpy_d2h(host.ctypes.data, buf.ptr, host.nbytes, None)
            return host

        if e == "laplace":
            return [run(lambda p: lib.laplace(info.ref, dev.ptr, p, layout, None))], None
        if e == "laplace_scaled":
            return [run(lambda p: lib.laplace_scaled(info.ref, dev.ptr, p, c.opt("s1"), c.opt("s2"), None))], None
        if e == "laplace_euler":
            ydev = DeviceArray(info).set_valid(built.ydata)
            return [run(lambda p: lib.laplace_euler(info.ref, dev.ptr, ydev.ptr, p, c.opt("s1"), c.opt("s2"), None))], None
        if e == "cahn_hilliard_mu":
            return [run(lambda p: lib.cahn_hilliard_mu(info.ref, dev.ptr, p, c.param, None))], None
        if e == "gradient":
            return [run(lambda p: lib.gradient(info.ref, _abi.METHODS[c.opt("method")], dev.ptr, p, layout, None)).reshape((nd, *c.shape))], None
        if e == "gradient_squared":
            return [run(lambda p: lib.gradient_squared(info.ref, int(c.opt("central")), dev.ptr, p, layout, None))], None
        if e == "divergence":
            return [run(lambda p: lib.divergence(info.ref, _abi.METHODS[c.opt("method")], dev.ptr, p, layout, None))], None
        return [run(lambda p: lib.axis_derivative(info.ref, c.opt("axis"), c.opt("order"), _abi.METHODS[c.opt("method")], dev.ptr, p, layout, None))], None

    done = C.c_int(0)
    if e in ("diffusion_euler2", "diffusion_euler2_slab", "ch_fused_euler", "ch_fused_rhs"):
        info = GridInfo(grid.shape, grid.discretization, dtype)
        fc = convert_bcs(built.bcs_c)
        a, b = DeviceArray(info).set_valid(data), DeviceArray(info)
        if e == "diffusion_euler2":
            lib.diffusion_euler2(info.ref, fc.c, a.ptr, b.ptr, c.param, c.dt, C.byref(done), None)
        elif e == "diffusion_euler2_slab":
            # first and last slab of a non-periodic slowest axis: one side is the physical face, the other reads two real layers of the other half
            split, n0 = c.opt("split"), c.shape[0]
            lp = info.layer_pitch * dtype.itemsize
            for first, count, sides in [(1, split, 2), (split + 1, n0 - split, 3)]:
                sub = GridInfo((count, *c.shape[1:]), grid.discretization, dtype)
                f = _abi.FaceArray()
                for i in range(6):
                    f[i] = fc.c[i]
                f[0 if sides == 3 else 1].kind = _abi.BC_SKIP
                f[1].index1 -= first - 1
                lib.diffusion_euler2_slab(sub.ref, f, a.ptr + (first - 1) * lp, b.ptr + (first - 1) * lp, c.param, c.dt, sides, C.byref(done), None)
                if done.value != 1:
                    break
        else:
            fm = convert_bcs(built.bcs_mu)
            lib.cahn_hilliard_fused(info.ref, fc.c, fm.c, a.ptr, b.ptr, c.param, c.dt, 1 if e == "ch_fused_euler" else 0, C.byref(done), None)
        return [b.get_valid()], done.value

    if c.kind == "diffusion":
        eq = pde_hip.DiffusionPDE(c.param, bc=built.bc_c)
    else:
        eq = pde_hip.CahnHilliardPDE(c.param, bc_c=built.bc_c, bc_mu=built.bc_mu)
    spec = backend.make_rhs_spec(eq, pde_hip.ScalarField(grid, data, dtype=dtype))
    info = spec.info
    a, b = DeviceArray(info).set_valid(data), DeviceArray(info)
    if e == "rhs_scaled":
        lib.rhs_scaled(info.ref, spec.ref, a.ptr, b.ptr, c.dt, None)
        return [b.get_valid()], None
    if e == "euler_multi_2d":
        lib.euler_multi_2d(info.ref, spec.ref, a.ptr, b.ptr, c.dt, c.steps, C.byref(done), None)
        return [b.get_valid()], done.value
    if e == "euler_run":
        res = C.c_void_p()
        lib.euler_run(info.ref, spec.ref, a.ptr, b.ptr, c.dt, c.steps, C.byref(res), None)
        assert res.value in (a.ptr, b.ptr)
        return [(b if res.value == b.ptr else a).get_valid()], None
    work = [DeviceArray(info) for _ in range(7)]
    if e == "rk4_step":
        for _ in range(c.steps):
            lib.rk4_step(info.ref, spec.ref, a.ptr, ptr_array(work[:5]), c.dt, None)
        return [a.get_valid()], None
    assert e == "rkf45_attempt", e
    err = DeviceScalar()
    lib.rkf45_attempt(info.ref, spec.ref, a.ptr, b.ptr, ptr_array(work), c.dt, err.ptr, None)
    return [b.get_valid(), np.array(err.value())], None


def _compared(arr, mask):
    return arr[mask] if mask is not None else arr


def _assert_oracle_bits(got, oracle, mask, what):
    for g, o in zip(got, oracle):
        np.testing.assert_array_equal(_compared(np.asarray(g), mask), _compared(np.asarray(o), mask), err_msg=what)


def _three_modes(backend, built, oracle, reference, mask, single_build=False):
    """default mode, contracted, default again; returns (results of the contracted build, name of its instance)"""
    case = built.case
    try:
        backend.fastmath = False
        mark = _mark(backend)
        got, done = _device_run(backend, built)
        name = _name_since(backend, mark)
        assert done in (None, 1), "the entry point declined the case"
        _assert_oracle_bits(got, oracle, mask, "default mode")
        if _must_record_a_name(case):
            assert name, "no kernel instance was recorded"
        if case.opt("instance"):
            assert case.opt("instance") in name, f"the case is in the table for its {case.opt('instance')} instance: {name}"
        backend.fastmath = True
        on = C.c_int(0)
        backend._lib.get_fastmath(C.byref(on))
        assert on.value == 1
        mark = _mark(backend)
        fast, done = _device_run(backend, built)
        fast_name = _name_since(backend, mark)
        assert done in (None, 1), "the contracted build declined the case"
        if name:
            assert fast_name.startswith(name) and "fastmath" in fast_name, (name, fast_name)     # the same instance of the other build
        else:
            assert fast_name == ""
        for f, (ref, bound) in zip(fast, reference):
            assert np.isfinite(_compared(np.asarray(f, dtype=np.float64), mask)).all()
            n_over, ratio = excess(f, ref, bound, mask)
            print(f"{case.id}: |result - reference| / bound <= {ratio:.4f}")
            assert n_over == 0, f"{n_over} cells of the contracted build leave the rounding bound of the expression (|diff| / bound up to {ratio:.4g})"
        if case.bit_equal or single_build:
            _assert_oracle_bits(fast, oracle, mask, "nothing to contract: the oracle's bits")
    finally:
        backend.fastmath = None
        _ = backend._lib
    again, _ = _device_run(backend, built)
    _assert_oracle_bits(again, oracle, mask, "default mode restored")
    return fast, fast_name


@pytest.mark.parametrize("index", range(len(CASES)), ids=IDS)
def test_instance_in_both_builds(backend, monkeypatch, index):
    case = CASES[index]
    for key, value in case.env:
        monkeypatch.setenv(key, value)
    built = build_case(index)
    oracle, reference, mask = built.oracle(), built.reference(), built.mask()
    fast, name = _three_modes(backend, built, oracle, reference, mask, single_build=case.family == SINGLE_BUILD)
    rec = REPORT.setdefault(case.family, {"cases": 0, "ratio": {}, "differs": 0, "names": set()})
    rec["cases"] += 1
    rec["ratio"][case.dtype] = max(rec["ratio"].get(case.dtype, 0.0), worst_ratio(fast, reference, mask))
    rec["differs"] += any(not np.array_equal(_compared(np.asarray(f), mask), _compared(np.asarray(o), mask)) for f, o in zip(fast, oracle))
    if name:
        rec["names"].add(name.split(" [fastmath")[0])


@pytest.mark.parametrize("family", FAMILIES)
def test_it_is_another_build(backend, monkeypatch, family):
    """In every family some case that contraction can change has other bits than the oracle (not per case: a small one may coincide)."""
    try:
        backend.fastmath = True
        for index, case in enumerate(CASES):
            if case.family != family or case.bit_equal:
                continue
            for key, value in case.env:
                monkeypatch.setenv(key, value)
            built = build_case(index)
            fast, _ = _device_run(backend, built)
            mask = built.mask()
            if any(not np.array_equal(_compared(np.asarray(f), mask), _compared(np.asarray(o), mask)) for f, o in zip(fast, built.oracle())):
                return
    finally:
        backend.fastmath = None
        _ = backend._lib
    pytest.fail(f"{family}: the contracted build gave the oracle's bits in every case - is it really another build?")


NON_FINITE = {
    # test_hip_euler2.py: test_special_values_stay_bit_identical (its grid and faces; one infinity and one NaN in ordinary data - denormals and
    # huge magnitudes would leave the relative rounding model the bound rests on)
    "two-step": Case(family="launch_euler2", entry="diffusion_euler2", shape=(9, 8, 128), dtype="float64", bounds=bounds_of((9, 8, 128), lambda i: 0.7 + 0.1 * i),
                     periodic=(True, False, True), bc=("local",), param=0.6, dt=2e-3, steps=2, seed=31),
    # test_hip_euler4_image.py: test_non_finite_values_spread_as_in_the_oracle
    "four-step": Case(family="launch_euler4", entry="euler_run", shape=(17, 64, 128), dtype="float64", bounds=tuple((0.0, float(n)) for n in (17, 64, 128)),
                      periodic=(True,) * 3, bc=("set", "periodic"), param=1.0, dt=0.05, steps=4, seed=11, env=(("PDEHIP_EULER4", "1"),)),
}


@pytest.mark.parametrize("which", list(NON_FINITE))
def test_non_finite_values_under_contraction(backend, monkeypatch, which):
    """NaN and +-inf cells where the oracle has them; every finite cell within the bound of a reference that never saw the non-finite values:
    a finite cell of the oracle is one that no non-finite value reaches, so the same data with zeros in their place gives its reference."""
    case = NON_FINITE[which]
    for key, value in case.env:
        monkeypatch.setenv(key, value)
    built, clean = Built(case), Built(case)
    if which == "two-step":
        flat = built.data.reshape(-1)
        flat[flat.size // 3], flat[2 * flat.size // 3] = np.inf, np.nan
    else:
        built.data[5, 31, 63], built.data[9, 32, 64], built.data[0, 0, 0] = np.nan, np.inf, -np.inf
    clean.data = np.where(np.isfinite(built.data), built.data, 0.0)
    with np.errstate(all="ignore"):
        want = built.oracle()[0]
    finite = np.isfinite(want)
    assert 0 < np.isnan(want).sum() < want.size // 4 and np.isinf(want).any() and finite.sum() > want.size // 2   # the case is what it claims to be
    ref, bound = clean.reference()[0]
    assert excess(want, ref, bound, finite)[0] == 0      # (the reference of the finite cells is the oracle's)
    try:
        backend.fastmath = True
        fast, done = _device_run(backend, built)
        name = backend._lib.last_kernel_name().decode()
    finally:
        backend.fastmath = None
        _ = backend._lib
    assert done in (None, 1)
    assert "fastmath" in name and ("euler4_kernel" in name) == (which == "four-step"), name
    got = fast[0]
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.where(np.isinf(got), got, 0.0), np.where(np.isinf(want), want, 0.0))
    n_over, ratio = excess(got, ref, bound, finite)
    assert n_over == 0, f"{n_over} finite cells leave the bound (|diff| / bound up to {ratio:.4g})"
    again, _ = _device_run(backend, built)
    np.testing.assert_array_equal(again[0], want)


EXPRESSION = "laplace(c**3 - c - laplace(c))"


@pytest.mark.parametrize("compiled", [False, True], ids=["matched-to-the-class", "through-the-compiler"])
def test_expression_kernels_keep_their_modes_apart(backend, compiled):
    """One Euler step of an expression PDE in default mode, contracted, and in default mode again: the kernels of the two modes are cached under
    different keys (csrc/pdehip_jit.hip: mode_key).  First and third step are bit-equal to each other and to the step of CahnHilliardPDE; the
    contracted one lies within the Cahn-Hilliard bound.  `eq.solve` recognises the expression as CahnHilliardPDE and takes its hand-written
    sweep; `make_expression_rhs` sends it through the run-time compiler (tests/test_expressions.py), a kernel per arithmetic mode."""
    from pde_hip.rhs import _match_expression_rhs

    assert _match_expression_rhs(EXPRESSION, "c", {}) == (_abi.RHS_CAHN_HILLIARD, 1.0)
    shape, dt = (6, 8, 64), 1e-3
    case = Case(family="launch_euler2", entry="euler_run", shape=shape, dtype="float64", bounds=bounds_of(shape, lambda a: 0.8), periodic=(True,) * 3,
                bc=("set", "periodic"), kind="cahn_hilliard", param=1.0, dt=dt, steps=1, seed=13)
    built = Built(case)
    reference = built.reference()
    state = pde_hip.ScalarField(built.grid, built.data)

    def step(eq):
        if compiled and isinstance(eq, pde_hip.PDE):
            erhs = backend.make_expression_rhs(eq, state)      # (compiled for the mode that is current now)
            y, out = DeviceArray(erhs.info).set_valid(built.data), DeviceArray(erhs.info)
            erhs.apply(y, out, "euler", dt, 0.0)
            return out.get_valid()
        return eq.solve(state, t_range=dt, dt=dt, solver="euler", backend=backend, tracker=None).data

    try:
        backend.fastmath = False
        first = step(pde_hip.PDE({"c": EXPRESSION}, bc="periodic"))
        by_class = step(pde_hip.CahnHilliardPDE(1.0, bc_c="periodic", bc_mu="periodic"))
        backend.fastmath = True
        second = step(pde_hip.PDE({"c": EXPRESSION}, bc="periodic"))
        backend.fastmath = False
        third = step(pde_hip.PDE({"c": EXPRESSION}, bc="periodic"))
    finally:
        backend.fastmath = None
        _ = backend._lib
    np.testing.assert_array_equal(first, third)
    np.testing.assert_array_equal(by_class, built.oracle()[0])
    np.testing.assert_array_equal(first, by_class)
    assert np.isfinite(second).all()
    n_over, ratio = excess(second, *reference[0])
    assert n_over == 0, f"{n_over} cells of the contracted step leave the Cahn-Hilliard bound (|diff| / bound up to {ratio:.4g})"
    assert np.abs(second - built.data).max() > 1e-6      # a step that did nothing must not pass
    # the contracted step really ran another kernel: 3072 cells of a fused cubic and two Laplacians do not all coincide with the exact build
    assert not np.array_equal(second, first), "the step under fastmath has the default mode's bits: did it run the kernel of the other mode?"
