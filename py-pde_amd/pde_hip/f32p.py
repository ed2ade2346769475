"""The pure-fp32 arithmetic mode of fp32 fields (``backend.f32_arithmetic = "fp32"``): what it serves and what it refuses.

Contract and reference lines: ``include/pdehip.h`` ("the PURE-fp32 arithmetic mode"), DESIGN.md §4.10.  The mode is captured when an
operator or a stepper is MADE and travels per call, by the choice of entry point (``pdehip_laplace_f32p`` / ``pdehip_euler_run_f32p``);
the library keeps no state.  Served: the 3 / 5 / 7-point Laplacian, and the fixed-step Euler loop of ``DiffusionPDE`` without noise or
hooks on one device whose axes are each periodic or zero-derivative.  Every other STENCIL computation on an fp32 field raises
``NotImplementedError`` in this mode - there is no silent return to fp64 registers; data movement, ghost cells, reductions and
interpolation are not stencil arithmetic and keep working.  fp64 fields are not affected.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi

MODES = ("fp64", "fp32")
OPTION = "backend.hip.f32_arithmetic"
ENTRY_POINTS = ("laplace_f32p", "euler_run_f32p", "f32p_supported")


def check_mode(value) -> str:
    """``"fp64"`` or ``"fp32"``; anything else is a ``ValueError``."""
    if isinstance(value, str) and value in MODES:
        return value
    msg = f"{OPTION} must be one of {', '.join(repr(m) for m in MODES)} (got {value!r})"
    raise ValueError(msg)


def is_f32(dtype) -> bool:
    return dtype is not None and np.dtype(dtype) == np.dtype(np.float32)


def refusal(what: str, why: str = "") -> str:
    """Message of every refusal: names the operator / solver and the option."""
    return f"hip backend: {what} has no pure-fp32 kernel ({OPTION} = 'fp32'){': ' + why if why else ''}; use the default 'fp64' arithmetic for it"


def require_entry_points(lib) -> None:
    """A library without the new symbols (the host library of the CPU tests) is refused like before they existed."""
    if not lib.has(*ENTRY_POINTS):
        missing = sorted("pdehip_" + name for name in ENTRY_POINTS if name in lib.missing)
        msg = f"hip backend: the loaded library does not export {', '.join(missing)}: no {OPTION} = 'fp32' with it"
        raise NotImplementedError(msg)


def laplace(backend, lib, arr, out) -> None:
    """``pdehip_laplace_f32p`` on two full device arrays (ghost cells of ``arr`` set by the caller; the entry points were checked when the
    operator was made)."""
    lib.laplace_f32p(arr.info.ref, arr.ptr, out.ptr, _abi.OUT_FULL, backend.stream)


def operator_refusal(backend, name: str, op_no_bc) -> str | None:
    """Made in "fp32" mode: the message with which this operator refuses fp32 fields, or None for the operators the mode serves."""
    if getattr(op_no_bc, "_f32p_ok", False):
        if backend.fastmath:
            return refusal(f"operator `{name}`", "`fastmath` contracts operations, this mode rounds every one of them")
        return None
    label = getattr(op_no_bc, "__name__", name)
    detail = f" ({label})" if label not in (name, "") else ""
    return refusal(f"operator `{name}`{detail}")


def complex_refusal(name: str) -> str:
    """complex64 fields are pairs of fp32 parts: the mode has no contract for them (the reference's torch backend computes them in complex
    arithmetic), so they are refused rather than sent part by part through either arithmetic."""
    return refusal(f"operator `{name}` on a complex64 field", "the mode is defined for real float32 fields")


def guard_operator(op, message: str, dtype_of):
    """``op`` refusing fp32 operands with ``message`` before anything is launched; other types pass through."""

    def guarded(arr, *args, **kwargs):
        if is_f32(dtype_of(arr)):
            raise NotImplementedError(message)
        return op(arr, *args, **kwargs)

    for attr in ("grid", "_hip_operator", "__name__"):
        if hasattr(op, attr):
            try:
                setattr(guarded, attr, getattr(op, attr))
            except (AttributeError, TypeError):
                pass
    return guarded


def stepper_refusal(backend, solver, state, scheme, has_noise: bool, has_hook: bool) -> str | None:
    """Why the pure-fp32 Euler loop cannot take this run (None: it can, as far as that is decided without the face tables)."""
    eq = solver.pde
    eq_name = type(eq).__name__
    solver_name = getattr(scheme, "name", type(solver).__name__)
    if backend.fastmath:
        return refusal(f"solver {solver_name}", "`fastmath` contracts operations, this mode rounds every one of them")
    if not any(c.__name__ == "DiffusionPDE" for c in type(eq).__mro__):
        return refusal(f"equation {eq_name}", "only DiffusionPDE has a pure-fp32 time loop")
    if scheme.kind != "euler" or scheme.adaptive:
        return refusal(f"solver {solver_name}", "only the fixed-step explicit Euler scheme has a pure-fp32 time loop")
    if has_noise or getattr(eq, "is_sde", False):
        return refusal(f"solver {solver_name} with noise")
    if has_hook:
        return refusal(f"solver {solver_name} with a post-step hook")
    if state.__class__.__name__ != "ScalarField":
        return refusal(f"solver {solver_name} on a {state.__class__.__name__}")
    return None


def make_euler_stepper(backend, lib, spec, dt: float, info: dict, hand_back):
    """``pdehip_euler_run_f32p``: one C call per call of the stepper (twin of ``make_class_fixed_stepper``)."""
    from .device import DeviceArray

    require_entry_points(lib)
    ginfo = spec.info
    answer = C.c_int(0)
    lib.f32p_supported(ginfo.ref, spec.ref, C.byref(answer))          # dry run: nothing is launched
    if not answer.value:
        raise NotImplementedError(refusal("solver euler with these boundary conditions", lib.last_error()))
    work = DeviceArray(ginfo)
    stream = backend.stream

    def fixed_stepper(state_data, t_start: float, t_end: float):
        steps = max(1, round((t_end - t_start) / dt))
        res = C.c_void_p()
        lib.euler_run_f32p(ginfo.ref, spec.ref, state_data.ptr, work.ptr, dt, steps, C.byref(res), stream)
        hand_back(lib, stream, state_data, res.value)
        info["steps"] += steps
        return state_data, t_start + (steps - 1) * dt + dt

    fixed_stepper.keepalive = (work, spec)   # type: ignore[attr-defined]
    return fixed_stepper
