"""What runs between the steps of a stepper, as :class:`NoiseHookMixin` of the backend: the noise increment of an Euler-Maruyama step
(``make_gaussian_noise``, ``_make_noise_step``) and the PDE's post-step hook (``_make_host_post_step``: traced onto the device through
``pde_hip/hooks.py`` where that is possible, else a host round trip per step).  :func:`variance_noise_step` is shared with the decomposed steppers.

Reference: ``pde/pdes/base.py:160-208``, ``:634-722``, ``pde/solvers/euler.py:66-147``, ``pde/solvers/milstein.py:103-127``, ``pde/backends/base.py:714-726``.
"""

from __future__ import annotations

import ctypes as C
import logging
import os

import numpy as np

from .device import DeviceArray, ptr_array

_logger = logging.getLogger("pde_hip.backend")


def draw_seed(rng) -> int:
    """Seed of the device generator from the equation's ``rng``, like the torch backend (pde/backends/torch/backend.py:619)."""
    return int((rng if rng is not None else np.random.default_rng()).integers(0, 2**32))


def variance_noise_step(lib, stream, info, eq, ncomp: int, grid, dt: float, who: str, first: int = 0, share_seed=int):
    """``add_noise(array, prev=None, t=0.0)`` of an Euler-Maruyama step for additive Gaussian white noise of constant variance ``eq.noise``:
    ``state += sqrt(dt) * sqrt(noise / cell_volume) * dW`` with dW from the device generator (``pdehip_add_gaussian_noise``), on the
    arrays of ``info`` - the whole ``grid`` or the box of a rank, which draws from its own part of the counter space (``first``) with
    the seed all ranks agree on (``share_seed``)."""
    try:
        # one variance for all fields or one per field of a collection (pde/pdes/pde.py:266-281, base.py:634-722)
        noise = np.broadcast_to(np.asarray(getattr(eq, "noise", 0), dtype=float), (ncomp,))
    except ValueError:
        noise = None
    if noise is None or (noise < 0).any():
        msg = f"{who} needs one non-negative noise variance per field"
        raise NotImplementedError(msg)
    cell_volume = float(np.prod(grid.discretization))
    cells = int(np.prod(grid.shape))
    scales = [float(np.sqrt(dt) * np.sqrt(v / cell_volume)) for v in noise]
    seed, counter = share_seed(draw_seed(getattr(eq, "rng", None))), [0]

    def add_noise(arr: DeviceArray, prev=None, t: float = 0.0) -> None:
        flat = arr.flat() if ncomp > 1 else None
        for k in range(ncomp):
            # every field its own variance (none: nothing to add); the cell offset keeps the fields' random streams apart
            if scales[k] != 0:
                ptr = arr.ptr if flat is None else flat.component(k).ptr
                lib.add_gaussian_noise(info.ref, 1, ptr, scales[k], seed, counter[0], first + k * cells, stream)
        counter[0] += 1

    return add_noise


class NoiseHookMixin:
    """Noise and post-step hooks of :class:`~pde_hip.backend.HipBackendMixin`."""

    def make_gaussian_noise(self, field, *, rng=None):
        """``noise() -> DeviceArray`` of independent standard-normal values with the shape of ``field.data``
        (``BackendBase.make_gaussian_noise``, pde/backends/base.py:714-726; numba: pde/backends/numba/backend.py, torch:
        pde/backends/torch/backend.py:603-625).  Device generator of ``pdehip_add_gaussian_noise`` (Philox4x32-10 +
        Box-Muller) seeded from ``rng`` like the torch backend; every call advances the counter."""
        grid = field.grid
        info = self.grid_info(grid, field.dtype)
        nd = grid.num_axes
        comp_shape = tuple(field.data.shape[: field.data.ndim - nd])
        seed, counter, lib = draw_seed(rng), [0], self._lib

        def noise() -> DeviceArray:
            out = DeviceArray(info, comp_shape)   # zero-initialised
            lib.add_gaussian_noise(info.ref, out.ncomp, out.ptr, 1.0, seed, counter[0], 0, self.stream)
            counter[0] += 1
            return out

        return noise

    def _make_noise_step(self, solver, scheme, state):
        """Noise increment of an Euler-Maruyama step as ``add_noise(array: DeviceArray)``, or None for deterministic equations.

        Covers the reference's standard case — additive Gaussian white noise of constant variance ``eq.noise``
        (``SDEBase.make_noise_variance``, ``pde/pdes/base.py:634-722``) in ``EulerSolver`` with a fixed step
        (``pde/solvers/euler.py:66-147``): ``state += sqrt(dt) * sqrt(noise / cell_volume) * dW``; additive noise has no drift
        correction in any interpretation.  dW comes from the device generator of ``pdehip_add_gaussian_noise`` seeded from
        ``eq.rng`` (like the torch backend, ``pde/backends/torch/backend.py:603-625``); realisations are therefore not those
        of the numba backend, only their statistics agree.  Everything else (state-dependent variance, noise realisations,
        Milstein, adaptive steps) raises like the reference / ``NotImplementedError``."""
        eq = solver.pde
        if not getattr(eq, "is_sde", False):
            return None
        if scheme.adaptive:
            msg = "Cannot use adaptive stepping with stochastic equation"   # pde/solvers/base.py:446-449
            raise RuntimeError(msg)
        if scheme.kind != "euler":      # (EulerSolver, ExplicitSolver, MilsteinSolver)
            msg = f"Backend `{self.name}` does not support stochastic equations with {scheme.name}"
            raise NotImplementedError(msg)
        custom_variance = False
        for cls in type(eq).__mro__:
            if "make_noise_variance" in vars(cls):
                custom_variance = cls.__name__ not in {"SDEBase", "PDEBase"}
                break
        if getattr(eq, "use_noise_realization", False):
            # Noise given as a REALISATION (pde/pdes/base.py:578, pde/solvers/euler.py:99-127: `state += sqrt(dt) * realization(state_old, t)`):
            # arbitrary Python on host arrays - the reference's own device backend refuses it (pde/backends/torch/_solvers.py:312-314).  Here:
            # a host round trip per step (the old state down, the realisation up), warned like the hooks that cannot be traced.
            realization = eq.make_noise_realization(state, backend=self)
            _logger.warning("noise realisations of %s are user code on host arrays: the state crosses PCIe twice per step", type(eq).__name__)
            dt_sqrt = (C.c_double * 1)(float(np.sqrt(float(solver.info["dt"]))))
            has_var = not np.allclose(np.asarray(getattr(eq, "noise", 0), dtype=float), 0, atol=1e-14)
            if getattr(eq, "use_noise_variance", True) and has_var:
                msg = f"Backend `{self.name}`: a noise variance next to a noise realisation is not supported"
                raise NotImplementedError(msg)
            ninfo = self.grid_info(state.grid, state.dtype)
            comp = tuple(np.shape(state.data))[: np.ndim(state.data) - len(ninfo.shape)]

            def add_realization(arr: DeviceArray, prev=None, t: float = 0.0) -> None:
                host_old = (prev if prev is not None else arr).get_valid(stream=self.stream)
                noise = realization(host_old, t)
                if noise is None:
                    return
                up = DeviceArray(ninfo, comp).set_valid(np.ascontiguousarray(np.broadcast_to(noise, host_old.shape), dtype=ninfo.dtype), self.stream)
                self._lib.lincomb(ninfo.ref, int(np.prod(comp)) if comp else 1, arr.ptr, arr.ptr, 1, dt_sqrt, ptr_array([up]), self.stream)

            solver.info["stochastic"] = True
            return add_realization
        if not getattr(eq, "use_noise_variance", True):
            msg = f"Backend `{self.name}`: a stochastic equation without noise variance and without noise realisation"
            raise NotImplementedError(msg)
        if custom_variance:
            return self._make_traced_noise_step(solver, scheme, state)
        grid = state.grid
        nd = grid.num_axes
        ncomp = int(np.prod(state.data.shape[: state.data.ndim - nd])) if state.data.ndim > nd else 1
        add_noise = variance_noise_step(self._lib, self.stream, self.grid_info(grid, state.dtype), eq, ncomp, grid, float(solver.info["dt"]),
                                        who=f"Backend `{self.name}`")
        solver.info["stochastic"] = True
        return add_noise

    def _make_traced_noise_step(self, solver, scheme, state):
        """Euler-Maruyama increment for a noise variance that depends on the field (``make_noise_variance`` overridden by the user,
        ``pde/pdes/base.py:634-722``; multiplicative noise): ``add_noise(new, old, t)``.

        The user's function ``noise_variance(state_data, t)`` is Python; like ``user_funcs`` it is TRACED once with a symbolic field
        and compiled into one pointwise kernel that applies the reference's update (``pde/solvers/euler.py:112-141``) to the
        deterministic step: ``new += sqrt(dt) * sqrt(variance(old, t) / cell_volume) * dW`` and, for interpretations other than
        Ito, ``+ 0.5 * dt * alpha * d variance / d field (old, t) / cell_volume``.  The variance is evaluated on the state BEFORE
        the step, like the reference does.  dW comes from the device generator (see :meth:`_make_noise_step`)."""
        import sympy as sp

        from .expr import ExpressionPlan, ExpressionRhs

        eq = solver.pde
        grid = state.grid
        if state.__class__.__name__ != "ScalarField":
            msg = f"Backend `{self.name}`: a noise variance that depends on the field is supported for scalar fields"
            raise NotImplementedError(msg)
        alpha = float(getattr(eq, "_noise_drift_factor", 0.0))
        milstein = scheme.milstein     # pde/solvers/milstein.py:103-127: always with the derivative
        need_diff = alpha != 0 or milstein
        c, t = sp.Symbol("pdehip_c", real=True), sp.Symbol("t", real=True)
        try:
            try:
                func = eq.make_noise_variance(state, backend=self, ret_diff=need_diff)
            except TypeError:
                func = eq.make_noise_variance(state, backend=self)
            traced = func(c, t)
            var, dvar = (traced if need_diff else (traced, 0))
            var, dvar = sp.sympify(var), sp.sympify(dvar)
        except NotImplementedError:
            raise
        except Exception as err:   # noqa: BLE001 - whatever the user's code raises on symbolic input
            msg = (f"hip backend: the noise variance of {eq.__class__.__name__} cannot be traced symbolically ({type(err).__name__}: {err}); "
                   "it must work on sympy expressions (arithmetic, sympy functions)")
            raise NotImplementedError(msg) from err
        unknown = (var.free_symbols | dvar.free_symbols) - {c, t}
        if unknown:
            msg = f"hip backend: the noise variance of {eq.__class__.__name__} depends on {sorted(map(str, unknown))}"
            raise NotImplementedError(msg)
        info = self.grid_info(grid, state.dtype)
        cell_volume = float(np.prod(grid.discretization))
        dt = float(solver.info["dt"])
        # sqrt(dt) * sqrt(var / V) * dW, the operations of pde/solvers/euler.py:132-133 in their order
        text = f"pdehip_unew + {float(np.sqrt(dt))!r} * sqrt(({sp.sstr(var)}) * {1.0 / cell_volume!r}) * pdehip_dw"
        if alpha != 0:
            text += f" + {0.5 * dt * alpha!r} * ({sp.sstr(dvar)}) * {1.0 / cell_volume!r}"
        if milstein:
            # + 0.25 * dvar / V * (dW**2 - dt) with dW = sqrt(dt) * xi   (pde/solvers/milstein.py:119-125)
            text += f" + 0.25 * ({sp.sstr(dvar)}) * {1.0 / cell_volume!r} * (({float(np.sqrt(dt))!r} * pdehip_dw)**2 - {dt!r})"
        plan = ExpressionPlan(text, "pdehip_c", {}, axes=tuple(grid.axes), aux=("pdehip_unew", "pdehip_dw"))
        dw = DeviceArray(info)
        erhs = ExpressionRhs(self, plan, info, {}, {"pdehip_unew": dw, "pdehip_dw": dw})   # (`unew` is bound per step)
        seed, counter, lib = draw_seed(getattr(eq, "rng", None)), [0], self._lib

        def add_noise(arr: DeviceArray, prev=None, t: float = 0.0) -> None:
            if prev is None:
                msg = "internal: a field-dependent noise variance needs the state before the step"
                raise RuntimeError(msg)
            lib.memset(dw.ptr, 0, dw.nbytes, self.stream)
            lib.add_gaussian_noise(info.ref, 1, dw.ptr, 1.0, seed, counter[0], 0, self.stream)
            counter[0] += 1
            erhs.aux["aux:pdehip_unew"] = arr
            erhs.apply(prev, arr, "rate", 0.0, float(t))     # pointwise, in place on the new state

        add_noise.keepalive = (erhs, dw)   # type: ignore[attr-defined]
        solver.info["stochastic"] = True
        return add_noise

    def _make_host_post_step(self, solver, state):
        """The PDE's post-step hook (``pde/solvers/base.py:191-232``, ``pde/pdes/base.py:160-208``) as
        ``post_step(array: DeviceArray, t) -> DeviceArray``, or None when the PDE defines none.

        Hooks are user code written against numpy arrays (``state_data[i] = 1``, ``raise StopIteration`` ...), so they run
        on the HOST: the valid data is downloaded, handed to the hook, and uploaded again after every step — a full PCIe
        round trip per step, logged once as a warning.  ``StopIteration`` propagates to the controller
        (``pde/solvers/controller.py:235-240``); ``solver.info["post_step_data"]`` is kept up to date."""
        make_hook = getattr(solver.pde, "make_post_step_hook", None)
        if make_hook is None or not getattr(solver, "_use_post_step_hook", True):
            solver.info.setdefault("post_step_data", None)
            return None
        try:
            try:
                hook, data = make_hook(state, backend="numpy")
            except TypeError:
                hook, data = make_hook(state)          # mirror classes without the `backend` argument
        except NotImplementedError:
            solver.info["post_step_data"] = None   # no hook defined: the normal case
            return None
        solver.info["post_step_data"] = data
        device_hook = self._make_device_post_step(solver, state, hook, data)
        if device_hook is not None:
            return device_hook
        _logger.warning("post-step hook of %s runs on the host: the state crosses PCIe twice per step", solver.pde.__class__.__name__)

        def post_step(arr: DeviceArray, t: float) -> DeviceArray:
            host = arr.get_valid(stream=self.stream)
            try:
                result = hook(host, t, solver.info["post_step_data"])
            except StopIteration:
                # a hook may have changed the state IN PLACE before it ended the run (the reference's arrays are the state
                # itself, tests/pdes/test_pde_class.py:546-566): what it left behind is the final state
                arr.set_valid(np.asarray(host, dtype=arr.dtype), self.stream)
                raise
            if result is not None:                      # hooks may work in place and return nothing (older signature)
                host, solver.info["post_step_data"] = result
            arr.set_valid(np.asarray(host, dtype=arr.dtype), self.stream)
            return arr

        return post_step

    def _make_device_post_step(self, solver, state, hook, data):
        """The hook as ONE run-time compiled pointwise pass on the device (``pde_hip/hooks.py``: the hook is traced once with a symbolic
        array - masked assignment, ``np.clip`` / ``np.where`` / ``np.minimum`` ..., arithmetic with ``t``), or None when it cannot be
        traced (reductions, control flow on values, hook data that changes, states that are not one real scalar field): then the host
        round trip below.  The reference compiles hooks into its jitted loops (``pde/backends/numba/_solvers.py:22-64``).
        The trace CALLS the hook once with a symbolic array.  By default only hooks given as ``PDE(..., post_step_hook=f)`` are traced - the
        form the reference hands to its backend's compiler (``pde/pdes/pde.py:691-706``: compiled code has no Python side effects); a
        class that overrides ``make_post_step_hook`` may count calls or collect data in Python and keeps the host path unless
        ``PDEHIP_DEVICE_HOOKS=1`` asks for the trace (``=0``: never)."""
        mode = os.environ.get("PDEHIP_DEVICE_HOOKS", "auto")
        if mode == "0" or state.__class__.__name__ != "ScalarField" or np.dtype(state.dtype).kind != "f":
            return None
        if mode != "1":
            eq = solver.pde
            plain = getattr(eq, "post_step_hook", None) is not None and not any(
                "make_post_step_hook" in vars(c) for c in type(eq).__mro__ if c.__name__ not in ("PDE", "PDEBase", "object") and c.__module__ != "pde.pdes.pde")
            if not plain:
                return None
        from .expr import ExpressionPlan, ExpressionRhs
        from .hooks import trace_hook

        expr = trace_hook(hook, data, tuple(state.grid.shape), state.dtype)
        if expr is None:
            return None
        try:
            plan = ExpressionPlan(expr, "c", {}, axes=tuple(state.grid.axes))
            if plan.operators_used or plan.aux_used or len(plan.passes) != 1:
                return None
            erhs = ExpressionRhs(self, plan, self.grid_info(state.grid, state.dtype), {}, {})
        except Exception:  # noqa: BLE001 - an expression the planner / printer cannot take: host path
            return None
        _logger.info("post-step hook of %s runs on the device as `c <- %s`", solver.pde.__class__.__name__, expr)

        def post_step(arr: DeviceArray, t: float) -> DeviceArray:
            # IN PLACE: the pass is pointwise (no operators: checked above), every cell is read as the centre value only by the
            # thread that then writes it.  (Round 4 wrote into a recycled "spare" array and returned that: across stepper calls the
            # spare could be the caller's own `state_data`, i.e. the stepper's next output buffer - `cur is nxt`, an in-place
            # stencil sweep; ADVICE r4 high.  The hook now never hands out an array the stepper does not already hold as `cur`.)
            erhs.apply(arr, arr, "rate", 0.0, float(t))
            return arr

        post_step.on_device = True  # type: ignore[attr-defined]
        post_step.expression = expr  # type: ignore[attr-defined]
        return post_step
