"""Time steppers of the backend.  Module-level builders put the loops together from what they use - the library, a stream, a right-hand-side
evaluator (:class:`~pde_hip.rhs.RhsEvaluator`), a :class:`SolverScheme`, the step parameters and the ``info`` dict they update;
:class:`StepperMixin` (``make_inner_stepper`` / ``make_stepper``) gathers those from a backend, a solver and a state, and
``DecomposedExpressionStepper`` calls the same builders for the box of a rank.  Noise and post-step hooks: ``pde_hip/noise_hooks.py``.

Reference: ``pde/solvers/euler.py:66-283``, ``pde/solvers/runge_kutta.py:29-156``, ``pde/backends/numba/_solvers.py:22-466``, ``pde/backends/base.py:728-755``.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

from . import _abi
from .device import DeviceArray, DeviceBuffer, DeviceScalar, ptr_array
from .faces import real_dtype_of
from .resident import ResidentState, _config_get
from .rhs import SpecRhs

# Runge-Kutta-Fehlberg 4(5), pde/solvers/runge_kutta.py:124-153 (the C loops hold the same numbers: csrc/pdehip_rk_loops.h)
RKF45_B = [[1 / 4], [3 / 32, 9 / 32], [1932 / 2197, -7200 / 2197, 7296 / 2197], [439 / 216, -8.0, 3680 / 513, -845 / 4104],
           [-8 / 27, 2.0, -3544 / 2565, 1859 / 4104, -11 / 40]]
RKF45_A = [0.0, 1 / 4, 3 / 8, 12 / 13, 1.0, 1 / 2]
RKF45_NEW = [25 / 216, 1408 / 2565, 2197 / 4104, -1 / 5]                   # new state from k1, k3, k4, k5 (runge_kutta.py:150)
RKF45_ERR = [1 / 360, -128 / 4275, -2197 / 75240, 1 / 50, 2 / 55]          # error from k1, k3, k4, k5, k6 (runge_kutta.py:147)


class SolverScheme(NamedTuple):
    """What the stepper builders need to know about a solver, decided once by :func:`classify_solver`."""

    kind: str | None          # euler | runge-kutta | adams-bashforth | implicit | crank-nicolson; None: a solver this backend does not know
    adaptive: bool = False
    milstein: bool = False    # MilsteinSolver: Euler steps, with the derivative term of a field-dependent noise variance
    name: str = ""            # the solver's class name, for messages


def _fixedpoint_scheme(solver) -> int | None:
    """0 / 1 for the reference's implicit Euler / Crank-Nicolson solver, recognised by the name it is registered under and its
    parameters (not by the class name: any class may be called ``ImplicitSolver``), else None."""
    name = getattr(solver, "name", None)
    if not (hasattr(solver, "maxiter") and hasattr(solver, "maxerror")):
        return None
    if name == "implicit":
        return _abi.FIXEDPOINT_IMPLICIT
    if name == "crank-nicolson" and hasattr(solver, "explicit_fraction"):
        return _abi.FIXEDPOINT_CRANK_NICOLSON
    return None


def classify_solver(solver, has_fixedpoint=lambda: True) -> SolverScheme:
    """The one place that decides which scheme a solver object stands for: the two fixed-point solvers by :func:`_fixedpoint_scheme`
    (``has_fixedpoint()`` False: a library without their loops - they are then solvers like any other), the explicit ones by class
    name (the reference's and the mirror's classes both match).  Never raises: ``kind`` None is refused by the caller."""
    cls = solver.__class__.__name__
    kind = {_abi.FIXEDPOINT_IMPLICIT: "implicit", _abi.FIXEDPOINT_CRANK_NICOLSON: "crank-nicolson"}.get(_fixedpoint_scheme(solver))
    if kind is None or not has_fixedpoint():
        kind = {"EulerSolver": "euler", "ExplicitSolver": "euler", "MilsteinSolver": "euler", "RungeKuttaSolver": "runge-kutta",
                "AdamsBashforthSolver": "adams-bashforth"}.get(cls)
    return SolverScheme(kind, bool(getattr(solver, "adaptive", False)), cls == "MilsteinSolver", cls)


def _convergence_error(solver) -> type:
    """The exception of a step that did not converge: py-pde's own for its solvers, else the mirror's."""
    if type(solver).__module__.split(".")[0] == "pde":
        try:
            from pde.solvers.base import ConvergenceError
        except ImportError:
            pass
        else:
            return ConvergenceError
    from .solvers import ConvergenceError

    return ConvergenceError


def expr_loops_enabled() -> bool:
    """``PDEHIP_EXPR_LOOP=0`` keeps the loops of run-time compiled right-hand sides in Python (a debugging aid)."""
    return os.environ.get("PDEHIP_EXPR_LOOP") != "0"


def _work_arrays(erhs, count: int) -> list[DeviceArray]:
    """``count`` arrays with the component layout of the states ``erhs`` evaluates: systems carry a leading component axis, complex
    states planar (re, im) pairs (such arrays hand out complex host data, e.g. to hooks)."""
    shape = ((erhs.ncomp // 2, 2) if erhs.complex_pairs else (erhs.ncomp,)) if erhs.ncomp > 1 else ()
    return [DeviceArray(erhs.info, shape, complex_pairs=erhs.complex_pairs) for _ in range(count)]


def _hand_back(lib, stream, state_data: DeviceArray, result_ptr) -> None:
    """The result belongs in the caller's array: a copy when the rotation of the buffers ended on a work array."""
    if result_ptr != state_data.ptr:
        lib.memcpy_d2d(state_data.ptr, result_ptr, state_data.nbytes, stream)


def _make_lincomb(lib, stream, erhs):
    ginfo, ncomp = erhs.info, erhs.ncomp

    def lincomb(out, y, coefs, ks):
        cf = (C.c_double * len(coefs))(*coefs)
        lib.lincomb(ginfo.ref, ncomp, out.ptr, y.ptr, len(ks), cf, ptr_array(ks), stream)

    return lincomb


# --- steppers driven from Python around any evaluator: the update rules of the C steppers (pde/solvers/euler.py:172-175, -------------
# runge_kutta.py:52-61, :135-153); the Euler update / RK stage scaling is folded into the last pass where the evaluator can
def make_fixed_stepper(lib, stream, erhs, scheme: SolverScheme, dt: float, info: dict, post_step=None):
    """Fixed steps of Euler (two steps per sweep / the whole loop in C where the evaluator offers it) or RK4 (``rk_run`` / stage sweeps).
    ``post_step(array, t) -> array``: the PDE's post-step hook, after every step with the time the step started at
    (pde/solvers/base.py:266-272); with a hook every step is a single sweep."""
    ginfo, ncomp = erhs.info, erhs.ncomp
    is_rk = scheme.kind == "runge-kutta"
    work = _work_arrays(erhs, 5 if is_rk else 1)
    lincomb = _make_lincomb(lib, stream, erhs)
    cells = int(np.prod(ginfo.shape))
    can_two = ncomp == 1 and erhs.two_steps_possible
    wants_prev = getattr(post_step, "wants_prev", False)

    def rk4_step(y, t, dt):
        # every stage in one sweep where the kernels cover it (slope + the combination that follows, like
        # pdehip_rk4_step): the array of k4 serves as the second stage input, k4 itself stays in registers
        k1, k2, k3, k4, tmp = work
        if not erhs.apply_stage(y, k1, dt, t, 0, y, [], [], 0.5, tmp):
            lincomb(tmp, y, [0.5], [k1])
        if not erhs.apply_stage(tmp, k2, dt, t + 0.5 * dt, 0, y, [], [], 0.5, k4):
            lincomb(k4, y, [0.5], [k2])
        if not erhs.apply_stage(k4, k3, dt, t + 0.5 * dt, 0, y, [], [], 1.0, tmp):
            lincomb(tmp, y, [1.0], [k3])
        if not erhs.apply_stage(tmp, k4, dt, t + dt, 1, y, [k1, k2, k3], [], 0.0, y):
            lib.rk4_combine(ginfo.ref, ncomp, y.ptr, k1.ptr, k2.ptr, k3.ptr, k4.ptr, stream)

    def fixed_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        steps = max(1, round((t_end - t_start) / dt))
        cur, nxt = state_data, work[0]
        i = 0
        try:
            if post_step is None and erhs.has_loops and expr_loops_enabled():
                # the whole loop in ONE C call (captured as a hipGraph for long runs): a Python iteration per step costs 40-85 us
                # where the kernels of a small grid need 2-5 us.  Euler: pdehip_jit_euler_run (large grids whose expression runs
                # two steps per sweep keep that: Python overhead is noise there); RK4: pdehip_jit_rk_run (reference: the jitted
                # loop pde/backends/numba/_solvers.py:93-118 around pde/solvers/runge_kutta.py:29-66)
                if is_rk:
                    if erhs.rk_run(cur, None, work, None, dt, t_start, steps) is not None:
                        i = steps
                elif not (can_two and cells > (1 << 21)):
                    done = erhs.euler_loop(cur, nxt, dt, t_start, steps)
                    if done is not None:
                        if done is not cur:
                            cur, nxt = nxt, cur
                        i = steps
            while i < steps:
                t = t_start + i * dt
                if is_rk:
                    rk4_step(cur, t, dt)
                elif post_step is None and i + 2 <= steps and erhs.euler2(cur, nxt, dt):   # two steps per sweep (one-pass expressions)
                    cur, nxt = nxt, cur
                    i += 1
                else:
                    erhs.apply(cur, nxt, "euler", dt, t)
                    cur, nxt = nxt, cur
                i += 1
                if post_step is not None:
                    cur = post_step(cur, t, nxt) if wants_prev else post_step(cur, t)
        finally:
            # also when a hook ends the run with StopIteration: the caller's array holds the latest state
            _hand_back(lib, stream, state_data, cur.ptr)
            info["steps"] += i
        return state_data, t_start + (steps - 1) * dt + dt

    return fixed_stepper


def _make_attempt(lib, stream, erhs, is_rk: bool, work, err_dev, reduce_error):
    """``attempt(y, ynew, t, dt) -> error``: one RKF45 attempt (work: k1..k6, tmp) or the second half of an adaptive Euler attempt
    (work: rate, half step, slope scratch); complex states take one more array, the error field."""
    ginfo, ncomp = erhs.info, erhs.ncomp
    lincomb = _make_lincomb(lib, stream, erhs)
    A, B = RKF45_A, RKF45_B

    def attempt_complex(y, ynew, t, dt_step) -> float:
        """New state and error FIELD with the pointwise kernels, then max |error| as the modulus over the (re, im) pairs
        (pdehip_max_abs_pairs) - `np.abs(...).max()` of a complex array in the reference."""
        efield = work[-1]
        if is_rk:
            ks, tmp = work[:6], work[6]
            src = y
            for s_, b in enumerate(B):
                erhs.apply(src, ks[s_], "scaled", dt_step, t + A[s_] * dt_step)
                lincomb(tmp, y, b, ks[: s_ + 1])
                src = tmp
            erhs.apply(src, ks[5], "scaled", dt_step, t + A[5] * dt_step)
            lincomb(ynew, y, RKF45_NEW, [ks[0], ks[2], ks[3], ks[4]])
            cf = (C.c_double * 5)(*RKF45_ERR)
            lib.lincomb(ginfo.ref, ncomp, efield.ptr, None, 5, cf, ptr_array([ks[0], ks[2], ks[3], ks[4], ks[5]]), stream)
        else:
            rate, half, kmid = work[0], work[1], work[2]
            h = 0.5 * dt_step
            erhs.apply(half, kmid, "scaled", h, t + h)
            lincomb(ynew, half, [1.0], [kmid])              # step_small += 0.5 * dt * rate_midpoint
            lincomb(efield, y, [dt_step], [rate])            # step_large
            lincomb(efield, efield, [-1.0], [ynew])          # step_large - step_small
        lib.max_abs_pairs(ginfo.ref, ncomp // 2, efield.ptr, err_dev.ptr, stream)
        if reduce_error is not None:
            reduce_error(err_dev)
        return err_dev.value(stream)

    def attempt(y, ynew, t, dt_step) -> float:
        if is_rk:
            # stages 1-5: slope + next stage input in one sweep (inputs alternate between tmp and ynew, which is free
            # until the last sweep); stage 6: new state + error norm with k6 in registers (like pdehip_rkf45_attempt)
            ks, tmp = work[:6], work[6]
            src, dst = y, tmp
            for s_, b in enumerate(B):
                if not erhs.apply_stage(src, ks[s_], dt_step, t + A[s_] * dt_step, 0, y, ks[:s_], b[:s_], b[s_], dst):
                    lincomb(dst, y, b, ks[: s_ + 1])
                src, dst = dst, (ynew if dst is tmp else tmp)
            if not erhs.apply_stage(src, ks[5], dt_step, t + A[5] * dt_step, 2, y, [ks[0], ks[2], ks[3], ks[4]], [], 0.0, ynew, err_dev):
                lib.rkf45_combine(ginfo.ref, ncomp, y.ptr, ynew.ptr, ptr_array(ks), err_dev.ptr, stream)
        else:
            # second half of the reference's adaptive Euler attempt (pde/backends/numba/_solvers.py:385-394): `work[1]` holds
            # step_small = y + dt/2 * rate; the sweep adds dt/2 * rhs(step_small, t + dt/2) and takes the error norm against
            # step_large = y + dt * rate, which is never stored (stage kind 4)
            rate, half, kmid = work[0], work[1], work[2]
            h = 0.5 * dt_step
            if not erhs.apply_stage(half, kmid, h, t + h, 4, y, [rate, half], [dt_step, 0.0], 0.0, ynew, err_dev):
                lib.euler_adaptive_combine(ginfo.ref, ncomp, y.ptr, rate.ptr, dt_step, half.ptr, kmid.ptr, ynew.ptr, err_dev.ptr, stream)
        if reduce_error is not None:
            reduce_error(err_dev)     # MAX over the ranks of a decomposed run, on the device, NaN wins (pde/backends/base.py:678-712)
        return err_dev.value(stream)

    return attempt_complex if erhs.complex_pairs else attempt


def _adaptive_python_loop(lib, stream, erhs, is_rk: bool, work, ynew0, attempt, tolerance: float, dt_min: float, adjust_dt, info: dict, post_step):
    """The adaptive loop of pde/backends/numba/_solvers.py:240-281 around ``attempt``, one Python iteration per attempt."""
    lincomb = _make_lincomb(lib, stream, erhs)
    is_complex = erhs.complex_pairs

    def adaptive_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        dt_opt = float(info["dt"])
        t, steps = t_start, 0
        stats = info["dt_statistics"]
        cur, nxt = state_data, ynew0   # an accepted attempt swaps the roles (no copy of the field per step)
        # Adaptive Euler is the reference's own loop (pde/backends/numba/_solvers.py:374-433, pde/solvers/euler.py:222-280; C twin
        # csrc/pdehip_rk_loops.h `euler_adaptive_run`): the rate of the current state is carried from attempt to attempt and,
        # after an accepted attempt, evaluated at the time BEFORE `t += dt` - here lazily at the start of the next attempt, in
        # the sweep that also writes the first half step; with a hook eagerly, before the hook sees (and may change) the state.
        have_rate, t_rate = False, t_start
        try:
            while True:
                dt_step = max(min(dt_opt, t_end - t), dt_min)
                if not is_rk:
                    rate, half = work[0], work[1]
                    h = 0.5 * dt_step
                    if is_complex and not have_rate:
                        erhs.apply(cur, rate, "rate", 0.0, t_rate)
                        have_rate = True
                    if have_rate or not erhs.apply_stage(cur, rate, 1.0, t_rate, 0, cur, [], [], h, half):
                        lincomb(half, cur, [h], [rate])
                    have_rate = True
                error_rel = attempt(cur, nxt, t, dt_step) / tolerance
                if error_rel <= 1:
                    steps += 1
                    t_rate = t
                    t += dt_step
                    cur, nxt = nxt, cur
                    have_rate = False
                    if post_step is not None:
                        if not is_rk:
                            erhs.apply(cur, work[0], "rate", 0.0, t_rate)   # `rate = rhs_pde(step_small, t)` precedes the hook (:402-411)
                            have_rate = True
                        cur = post_step(cur, t)
                    stats.add(dt_step)
                if t < t_end:
                    dt_opt = adjust_dt(dt_step, error_rel)
                else:
                    break
        finally:
            _hand_back(lib, stream, state_data, cur.ptr)
            info["dt"] = dt_opt
            info["steps"] += steps
        return state_data, t

    return adaptive_stepper


def make_adaptive_stepper(lib, stream, erhs, scheme: SolverScheme, tolerance, dt_min, dt_max, info: dict, post_step=None, reduce_error=None):
    """Steps with error control: RKF45 or the reference's adaptive Euler.  The loop itself runs in C where the evaluator offers it
    (``rk_run`` with a control block: pde/backends/numba/_solvers.py:199-319 is jitted in the reference), else - hooks, integrals,
    function-valued conditions - in Python.  ``post_step``: after every accepted step, with the new time
    (pde/backends/numba/_solvers.py:262-270); ``reduce_error(err_dev)``: MAX of the error over the ranks of a decomposed run."""
    from .solvers import AdaptiveStatistics, OnlineStatistics, make_dt_adjuster

    is_rk, is_complex = scheme.kind == "runge-kutta", erhs.complex_pairs
    info["dt_adaptive"] = True
    info.setdefault("dt_statistics", OnlineStatistics())
    # RKF45: k1..k6, tmp; adaptive Euler: rate, half step, slope scratch; complex states: + the error field of the modulus norm
    work = _work_arrays(erhs, (7 if is_rk else 3) + (1 if is_complex else 0))
    err_dev, (ynew0,) = DeviceScalar(), _work_arrays(erhs, 1)
    attempt = _make_attempt(lib, stream, erhs, is_rk, work, err_dev, reduce_error)
    python_loop = _adaptive_python_loop(lib, stream, erhs, is_rk, work, ynew0, attempt, float(tolerance), float(dt_min),
                                        make_dt_adjuster(dt_min, dt_max), info, post_step)
    # (decomposed grids: the C loops reduce the error over the ranks themselves when the passes carry their exchange descriptor)
    reduces_in_c = reduce_error is None or erhs.reduces_error_in_loops
    if not (post_step is None and erhs.has_loops and reduces_in_c and expr_loops_enabled()):
        return python_loop
    ctl = _abi.Adaptive()
    ctl.tolerance, ctl.dt_min, ctl.dt_max = float(tolerance), float(dt_min), float(dt_max)
    loop_work = (work[:7] if is_rk else work[:3]) + ([work[-1]] if is_complex else [])
    in_c = [True]

    def adaptive_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        if not in_c[0]:
            return python_loop(state_data, t_start, t_end)
        ctl.t_start, ctl.t_end, ctl.dt = float(t_start), float(t_end), float(info["dt"])
        before = int(ctl.steps)
        try:
            # RKF45 (pdehip_jit_rk_run) or the reference's adaptive Euler loop (pdehip_jit_euler_adaptive_run) in one C call
            res = erhs.rk_run(state_data, ynew0, loop_work, err_dev, 0.0, 0.0, 0, ctl, euler_adaptive=not is_rk)
        finally:
            info["steps"] += int(ctl.steps) - before
            info["attempts"] = int(ctl.attempts)
        if res is None:     # not available for this right-hand side (integrals, function-valued conditions): the Python loop from now on
            in_c[0] = False
            return python_loop(state_data, t_start, t_end)
        _hand_back(lib, stream, state_data, res.ptr)
        info["dt"] = float(ctl.dt)
        info["dt_statistics"] = AdaptiveStatistics(ctl)
        return state_data, float(ctl.t_last)

    return adaptive_stepper


def make_adams_bashforth_stepper(lib, stream, erhs, dt: float, info: dict):
    """Two-step Adams-Bashforth (pde/solvers/adams_bashforth.py:31-70, pde/backends/numba/_solvers.py:121-196) around any evaluator.

    The reference re-evaluates ``rhs(state_prev, t - dt)`` in every step; it equals the rate of the step before bit for bit, so it is
    kept instead: one right-hand side per step - rate and update in one sweep where the evaluator has it (``ab2_step``: the class
    right-hand sides, the state ping-pongs), else two kernels in place."""
    ginfo, ncomp = erhs.info, erhs.ncomp
    rates = _work_arrays(erhs, 2)   # [current, previous], roles swap every step
    (tmp,) = _work_arrays(erhs, 1)
    minus_dt = (C.c_double * 1)(-dt)
    first = [True]

    def fixed_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        steps = max(1, round((t_end - t_start) / dt))
        if first[0]:
            # state_prev = state - dt * rhs(state, t)  ->  rate_prev = rhs(state_prev, t - dt)   (adams_bashforth.py:62-66)
            erhs.apply(state_data, rates[0], "rate", 0.0, float(t_start))
            lib.lincomb(ginfo.ref, ncomp, tmp.ptr, state_data.ptr, 1, minus_dt, ptr_array([rates[0]]), stream)
            erhs.apply(tmp, rates[1], "rate", 0.0, float(t_start) - dt)
            first[0] = False
        cur, nxt = state_data, tmp
        for i in range(steps):
            t = t_start + i * dt
            if erhs.ab2_step(cur, nxt, rates[0], rates[1], dt, t):
                cur, nxt = nxt, cur
            else:
                erhs.apply(cur, rates[0], "rate", 0.0, t)
                lib.ab2_combine(ginfo.ref, ncomp, cur.ptr, rates[0].ptr, rates[1].ptr, dt, stream)
            rates.reverse()
        _hand_back(lib, stream, state_data, cur.ptr)
        info["steps"] += steps
        return state_data, t_start + (steps - 1) * dt + dt

    return fixed_stepper


def make_fixedpoint_stepper(lib, stream, erhs, fp, dt: float, info: dict, error_cls: type, post_step=None):
    """The fixed-point loops of the library (``fp``: the filled ``pdehip_fixedpoint_t``): ``pdehip_fixedpoint_run`` for a class right-hand
    side (:class:`SpecRhs`), ``pdehip_jit_fixedpoint_run`` for the run-time compiled ones; with a hook one step per call, the hook in between."""
    who = "Implicit Euler" if fp.scheme == _abi.FIXEDPOINT_IMPLICIT else "Crank-Nicolson"
    spec = erhs.spec if isinstance(erhs, SpecRhs) else None
    ginfo, ncomp = erhs.info, erhs.ncomp
    # the state array and two iterates rotate; rate_t for Crank-Nicolson; the slope scratch only where a sweep cannot carry the update
    work = _work_arrays(erhs, 2) + [_work_arrays(erhs, 1)[0] if fp.scheme == _abi.FIXEDPOINT_CRANK_NICOLSON else None, None]
    nbytes = C.c_size_t(0)
    lib.fixedpoint_ctl_bytes(ginfo.ref, ncomp, C.byref(nbytes))
    ctl_dev = DeviceBuffer(nbytes.value)
    info["function_evaluations"] = 0
    info["iterations"] = []

    def call(state_data: DeviceArray, t: float, nsteps: int) -> None:
        """``nsteps`` steps from time ``t``, the new state in ``state_data``."""
        counts = (C.c_int32 * nsteps)()
        fp.iterations = C.cast(counts, C.POINTER(C.c_int32))
        fp.steps_done = 0
        fp.evaluations = 0
        result = C.c_void_p()
        while True:
            ptrs = (C.c_void_p * 4)(*[None if w is None else w.ptr for w in work])
            if spec is not None:
                spec.c.t = float(t)
                lib.fixedpoint_run(ginfo.ref, spec.ref, C.byref(fp), dt, nsteps, state_data.ptr, ptrs, ctl_dev.ptr, ctl_dev.nbytes, C.byref(result), stream)
            else:
                passes, fixed, nfixed, _keep = erhs.loop_desc("scaled")
                program = erhs.bc_program()
                lib.jit_fixedpoint_run(ginfo.ref, passes, len(passes), fixed, nfixed, ncomp, C.byref(fp), dt, float(t), nsteps, state_data.ptr, ptrs,
                                       ctl_dev.ptr, ctl_dev.nbytes, (1 if erhs.stage_sweeps else 0) | (2 if erhs.complex_pairs else 0),
                                       None if program is None else program.ptr, C.byref(result), stream)
            if fp.status != 2:
                break
            work[3] = _work_arrays(erhs, 1)[0]      # this right-hand side writes its slope to memory: one more array, then the same call again
            fp.evaluations = 0
        done = int(fp.steps_done)
        info["steps"] += done
        info["function_evaluations"] += int(fp.evaluations)
        info["iterations"].extend(counts[: done + (1 if fp.status == 1 else 0)])
        fp.iterations = None
        if fp.status == 1:
            raise error_cls(f"{who} step did not converge.")      # implicit.py:106-108, crank_nicolson.py:112-113
        _hand_back(lib, stream, state_data, result.value)

    def fixed_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        steps = max(1, round((t_end - t_start) / dt))
        if post_step is None:
            call(state_data, t_start, steps)
        else:
            for i in range(steps):
                t = t_start + i * dt
                call(state_data, t, 1)
                # pde/solvers/base.py:266-272: after every step, with the time it started at
                _hand_back(lib, stream, state_data, post_step(state_data, t).ptr)
        return state_data, t_start + (steps - 1) * dt + dt

    fixed_stepper.keepalive = (work, ctl_dev, spec, erhs, fp)   # type: ignore[attr-defined]
    return fixed_stepper


# --- the fused class right-hand sides: the loops of the library ------------------------------------------------------------------
def make_class_fixed_stepper(lib, stream, spec, is_rk: bool, dt: float, info: dict):
    """``pdehip_euler_run`` / ``pdehip_rk4_run`` (pde/backends/numba/_solvers.py:93-118): one C call per call of the stepper."""
    ginfo = spec.info
    work = [DeviceArray(ginfo) for _ in range(5 if is_rk else 1)]
    work_ptrs = ptr_array(work)

    def fixed_stepper(state_data: DeviceArray, t_start: float, t_end: float):
        steps = max(1, round((t_end - t_start) / dt))
        spec.c.t = float(t_start)    # time of the first step: faces with explicit time dependence follow it inside the C loop
        if is_rk:
            lib.rk4_run(ginfo.ref, spec.ref, state_data.ptr, work_ptrs, dt, steps, stream)
        else:
            res = C.c_void_p()
            lib.euler_run(ginfo.ref, spec.ref, state_data.ptr, work[0].ptr, dt, steps, C.byref(res), stream)
            _hand_back(lib, stream, state_data, res.value)
        info["steps"] += steps
        return state_data, t_start + (steps - 1) * dt + dt  # `t + dt` of the last iteration

    return fixed_stepper


def make_class_adaptive_stepper(lib, stream, spec, is_rk: bool, tolerance, dt_min, dt_max, info: dict):
    """The whole adaptive loop in ONE C call (the slab loop templates without a communicator and without neighbours = their serial
    use): RKF45 attempts inside the generic loop of pde/backends/numba/_solvers.py:249-281 (``pdehip_slab_rkf45_run``), or the
    reference's own adaptive Euler loop with the carried rate, :374-433 (``pdehip_slab_euler_adaptive_run``).  Stage sequence, error
    norm, accept / reject, controller and step statistics run in C; the host reads 8 bytes per attempt."""
    from .solvers import AdaptiveStatistics

    ginfo = spec.info
    work = [DeviceArray(ginfo) for _ in range(7 if is_rk else 3)]   # adaptive Euler: rate, half step, scratch
    work_ptrs = ptr_array(work)
    err_dev, ynew = DeviceScalar(), DeviceArray(ginfo)
    flags = C.c_int(0)
    lib.slab_flags_supported(ginfo.ref, spec.ref, -1, -1, C.byref(flags))
    ctl = _abi.Adaptive()
    ctl.tolerance, ctl.dt_min, ctl.dt_max = float(tolerance), float(dt_min), float(dt_max)
    info["dt_adaptive"] = True
    info["dt_statistics"] = AdaptiveStatistics(ctl)
    run = lib.slab_rkf45_run if is_rk else lib.slab_euler_adaptive_run

    def adaptive_loop(state_data: DeviceArray, t_start: float, t_end: float):
        ctl.t_start, ctl.t_end, ctl.dt = float(t_start), float(t_end), float(info["dt"])
        before = int(ctl.steps)
        res = C.c_void_p()
        try:
            run(None, ginfo.ref, spec.ref, -1, -1, flags.value, state_data.ptr, ynew.ptr, work_ptrs, err_dev.ptr, C.byref(ctl), C.byref(res), stream)
        finally:
            info["steps"] += int(ctl.steps) - before
            info["attempts"] = int(ctl.attempts)      # accepted + rejected (not kept by the reference; bench.py prices an attempt)
        _hand_back(lib, stream, state_data, res.value)
        info["dt"] = float(ctl.dt)
        return state_data, float(ctl.t_last)

    adaptive_loop.keepalive = (work, ynew, err_dev, spec)   # type: ignore[attr-defined]  (work_ptrs holds raw pointers only)
    return adaptive_loop


class StepperMixin:
    """The stepper-facing methods of :class:`~pde_hip.backend.HipBackendMixin`: they gather what the builders above take."""

    def _make_expression_stepper(self, solver, scheme: SolverScheme, erhs, post_step=None):
        """Euler / RK4 / RKF45 / adaptive Euler driven from Python around ``erhs`` with the parameters of ``solver``."""
        if scheme.adaptive:
            return make_adaptive_stepper(self._lib, self.stream, erhs, scheme, solver.tolerance, solver.dt_min, solver.dt_max, solver.info, post_step)
        return make_fixed_stepper(self._lib, self.stream, erhs, scheme, float(solver.info["dt"]), solver.info, post_step)

    def _make_fixedpoint_stepper(self, solver, state, scheme: SolverScheme, post_step=None):
        """Implicit Euler (``pde/solvers/implicit.py:74-110``) and Crank-Nicolson (``pde/solvers/crank_nicolson.py:80-113``): the
        reference's fixed-point iteration for the class right-hand sides, expressions, systems and complex states.  Iterations,
        convergence norm and stop test run on the device.  ``solver.info["function_evaluations"]`` counts the
        right-hand sides really evaluated (``n + 2`` / ``n + 3`` per step of ``n`` iterations), ``solver.info["iterations"]`` the iterations
        of every step.  ``PDEHIP_FIXEDPOINT_BATCH=<n>`` (or ``solver.batch``) fixes the number of iterations enqueued between two reads of
        the control block (default: the count of the step before plus one); results do not depend on it."""
        eq = solver.pde
        if solver.info.get("stochastic"):
            msg = f"Backend `{self.name}` does not support stochastic equations with {scheme.name}"
            raise NotImplementedError(msg)
        try:
            if np.dtype(state.dtype).kind == "c":
                msg = "complex state"
                raise NotImplementedError(msg)
            erhs = SpecRhs(self, self.make_rhs_spec(eq, state))
        except NotImplementedError as err:
            try:
                erhs = self.make_expression_rhs(eq, state)
            except NotImplementedError as err2:
                if any(c.__name__ in ("DiffusionPDE", "CahnHilliardPDE") for c in type(eq).__mro__):
                    raise err from err2
                raise
        if isinstance(erhs, SpecRhs) and erhs.spec.host_time_dependent:
            msg = (f"Backend `{self.name}`: {scheme.name} does not support boundary conditions given as Python functions of time "
                   "(conditions that are expressions of time are supported)")
            raise NotImplementedError(msg)
        if not isinstance(erhs, SpecRhs) and not all(p.loop_ok() for p in erhs.parts):
            msg = (f"Backend `{self.name}`: {scheme.name} needs a right-hand side that runs inside the device loops: no integrals, no "
                   "boundary conditions given as Python functions of time, no decomposed grids")
            raise NotImplementedError(msg)
        fp = _abi.FixedPoint()
        fp.scheme = _abi.FIXEDPOINT_IMPLICIT if scheme.kind == "implicit" else _abi.FIXEDPOINT_CRANK_NICOLSON
        fp.maxiter, fp.maxerror2 = int(solver.maxiter), float(solver.maxerror) ** 2
        fp.explicit_fraction = float(getattr(solver, "explicit_fraction", 0.0))
        batch = getattr(solver, "batch", None)
        fp.batch = int(batch if batch is not None else os.environ.get("PDEHIP_FIXEDPOINT_BATCH", "0"))
        return make_fixedpoint_stepper(self._lib, self.stream, erhs, fp, float(solver.info["dt"]), solver.info, _convergence_error(solver), post_step)

    def make_inner_stepper(self, solver, state):
        """Device-level stepper ``(state: DeviceArray, t_start, t_end) -> (DeviceArray, t_last)``.

        Fixed steps follow ``pde/backends/numba/_solvers.py:93-118``; the adaptive loop follows
        ``:240-281`` with ``_make_dt_adjuster`` (``pde/solvers/base.py:559-592``).
        """
        # (a library without the fixed-point loops - the host library of the CPU tests - refuses the two solvers like every solver it does not know)
        scheme = classify_solver(solver, lambda: self._lib.has("fixedpoint_ctl_bytes", "fixedpoint_run", "jit_fixedpoint_run"))
        post_step = self._make_host_post_step(solver, state)
        add_noise = self._make_noise_step(solver, scheme, state)
        if self.f32_arithmetic == "fp32" and np.dtype(state.dtype) == np.dtype(np.float32):
            # the pure-fp32 arithmetic mode (pde_hip/f32p.py): the Euler loop of DiffusionPDE, or a refusal - never fp64 registers
            from . import f32p

            why = f32p.stepper_refusal(self, solver, state, scheme, add_noise is not None, post_step is not None)
            if why is not None:
                raise NotImplementedError(why)
            f32p.require_entry_points(self._lib)
            spec = self.make_rhs_spec(solver.pde, state)
            if spec.host_time_dependent or spec.c.kind != _abi.RHS_DIFFUSION:
                raise NotImplementedError(f32p.refusal(f"solver {scheme.name} with these boundary conditions"))
            return f32p.make_euler_stepper(self, self._lib, spec, float(solver.info["dt"]), solver.info, _hand_back)
        if add_noise is not None:
            # Euler-Maruyama: deterministic Euler step, noise increment, then the hook (pde/solvers/euler.py:120-141)
            hook = post_step

            def post_step(arr, t, prev=None, _hook=hook):   # noqa: E306
                add_noise(arr, prev, t)      # (`prev`: the state before the step - a variance that depends on the field reads it)
                return arr if _hook is None else _hook(arr, t)

            post_step.wants_prev = True   # type: ignore[attr-defined]
        if scheme.kind in ("implicit", "crank-nicolson"):
            return self._make_fixedpoint_stepper(solver, state, scheme, post_step)
        if scheme.kind is None:
            msg = f"Backend `{self.name}` does not support solver {scheme.name}"
            raise NotImplementedError(msg)
        # (MilsteinSolver on a deterministic equation: kind "euler", the Euler steps of its base class - pde/solvers/milstein.py:29)
        is_ab = scheme.kind == "adams-bashforth"
        if post_step is not None and is_ab:
            msg = f"Backend `{self.name}` does not support post-step hooks with {scheme.name}"
            raise NotImplementedError(msg)
        try:
            if np.dtype(state.dtype).kind == "c":
                # complex states: the equation as a real system of the parts through the run-time compiled passes (pde_hip/complex_expr.py)
                if add_noise is not None:
                    msg = f"Backend `{self.name}` does not support noise on complex fields"
                    raise RuntimeError(msg)
                msg = "complex state"
                raise NotImplementedError(msg)
            spec = self.make_rhs_spec(solver.pde, state)
        except NotImplementedError as err:
            try:
                # expression PDEs (and complex states) around the run-time compiled right-hand side
                erhs = self.make_expression_rhs(solver.pde, state)
                if is_ab:
                    return make_adams_bashforth_stepper(self._lib, self.stream, erhs, float(solver.info["dt"]), solver.info)
                return self._make_expression_stepper(solver, scheme, erhs, post_step)
            except NotImplementedError as err2:
                if not is_ab and any(c.__name__ in ("DiffusionPDE", "CahnHilliardPDE") for c in type(solver.pde).__mro__):
                    raise err from err2    # the reason the class right-hand side was refused is the informative one
                raise
        if post_step is not None:
            # the hook runs on the host between steps: the steps are driven from here, one sweep each
            return self._make_expression_stepper(solver, scheme, SpecRhs(self, spec), post_step)
        if spec.host_time_dependent:
            # faces given as Python functions: their coefficient arrays come from the host before every right-hand side, so the
            # steps are driven from here.  (Expression faces are refreshed on the device inside the C loops: spec.c.t.)
            if is_ab:
                msg = f"Backend `{self.name}` does not support time-dependent boundary conditions with {scheme.name}"
                raise NotImplementedError(msg)
            return self._make_expression_stepper(solver, scheme, SpecRhs(self, spec))
        if is_ab:
            return make_adams_bashforth_stepper(self._lib, self.stream, SpecRhs(self, spec), float(solver.info["dt"]), solver.info)
        is_rk = scheme.kind == "runge-kutta"
        if not scheme.adaptive:
            return make_class_fixed_stepper(self._lib, self.stream, spec, is_rk, float(solver.info["dt"]), solver.info)
        if os.environ.get("PDEHIP_ADAPTIVE_LOOP", "1") != "0":
            return make_class_adaptive_stepper(self._lib, self.stream, spec, is_rk, solver.tolerance, solver.dt_min, solver.dt_max, solver.info)
        # the same loops driven from Python (PDEHIP_ADAPTIVE_LOOP=0: a debugging aid)
        return self._make_expression_stepper(solver, scheme, SpecRhs(self, spec))

    def make_stepper(self, solver, state):
        """``stepper(state_field, t_start, t_end) -> t_last`` mutating ``state.data`` (base.py:728-755).

        The reference's device template moves the whole state over PCIe in both directions on EVERY call, i.e. at every
        tracker interrupt (``pde/backends/torch/backend.py:654-662``).  Here the state stays RESIDENT on the device between
        the calls of one stepper (config ``resident_state``, default on): the host copy of the field is refreshed only
        when somebody actually reads ``state.data`` (a tracker that stores or plots, the caller after the run), and the
        device copy is refreshed only after such an access (the view handed out is writable).  A run with ``tracker=None``
        or progress-only trackers uploads once and downloads once.  See :class:`ResidentState`.
        """
        inner = self.make_inner_stepper(solver, state)
        # (the layout of the STATE as the field hands it out - a rank-2 field keeps its two tensor axes - where the work arrays of the
        # builders follow the evaluator; complex states: planar (re, im) pairs of the real type on the device)
        is_complex = np.dtype(state.dtype).kind == "c"
        info = self.grid_info(state.grid, real_dtype_of(state.dtype))
        comp_shape = tuple(np.shape(state.data))[: np.ndim(state.data) - len(info.shape)] + ((2,) if is_complex else ())
        # a FieldCollection hands out its sub-fields as separate objects viewing the same memory: reads of `state[0].data`
        # cannot be intercepted, so collections take the plain upload / download per call
        resident = bool(_config_get(getattr(self, "config", None), "resident_state", True)) and state.__class__.__name__ != "FieldCollection"
        dev_state = DeviceArray(info, comp_shape, complex_pairs=is_complex)
        if not resident:

            def stepper(state_field, t_start: float, t_end: float) -> float:
                dev_state.set_valid(state_field.data, self.stream)
                result, t_last = inner(dev_state, t_start, t_end)
                result.get_valid(out=state_field.data, stream=self.stream)
                return t_last

            return stepper

        def resident_stepper(state_field, t_start: float, t_end: float) -> float:
            link = ResidentState.attach(state_field, dev_state, self)
            link.push()                                   # uploads only if the host copy may have changed
            try:
                result, t_last = inner(dev_state, t_start, t_end)
                _hand_back(self._lib, self.stream, dev_state, result.ptr)   # steppers hand back the array they were given; be safe
            finally:
                link.device_advanced()                    # also when a post-step hook ends the run (StopIteration)
            return t_last

        resident_stepper.device_state = dev_state  # type: ignore[attr-defined]
        return resident_stepper
