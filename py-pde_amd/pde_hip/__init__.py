"""pde_hip — MI355X (gfx950) backend for py-pde's finite-difference + explicit-stepper hot path.

Layers (bottom up):
  * ``lib/libpdehip.so``  hand-written HIP kernels behind the C ABI of ``include/pdehip.h``
  * ``_abi`` / ``_lib``    ctypes binding (loud failure when the library or the GPU is missing)
  * ``device``            device-resident ghost-padded arrays (the backend's native array type)
  * ``backend``           ``HipBackend`` — py-pde's ``BackendBase`` plugin surface
  * ``grids`` / ``boundaries`` / ``fields`` / ``pdes`` / ``solvers``  stand-alone mirror of the
    reference classes that call into the backend (same names, argument meaning, errors), used when
    py-pde itself is not installed; ``pypde_plugin`` registers the backend with a real py-pde.
  * ``mesh`` / ``distributed``  slab decomposition + halo exchange over RCCL (one process per GPU)

Importing this package never touches the GPU; the first compute call does and raises if the
library or a device is missing (there is no CPU fallback).
"""

from . import operators as _operators
from .backend import HipBackend, get_backend
from .boundaries import BoundariesList
from .distribution import FieldHistogram, field_histogram, field_median, field_quantile
from .domains import FieldDomains, domain_properties, field_domains
from .fields import FieldCollection, ScalarField, Tensor2Field, VectorField
from .grids import CartesianGrid, UnitGrid
from .interpolation import interpolate_to_grid
from .pdes import (PDE, AllenCahnPDE, CahnHilliardPDE, DiffusionPDE, KleinGordonPDE, KPZInterfacePDE, KuramotoSivashinskyPDE,
                   SwiftHohenbergPDE, WavePDE)
from .poisson import solve_laplace_equation, solve_poisson_equation
from .projection import image_data, line_data, project, slice_field
from .smoothing import smooth
from .spectrum import FieldSpectrum, field_spectrum
from .statistics import FieldStatistics, field_statistics
from .solvers import Controller, ConvergenceError, CrankNicolsonSolver, EulerSolver, ExplicitSolver, ImplicitSolver, RungeKuttaSolver

_operators.register_all(HipBackend, CartesianGrid)

__all__ = [
    "PDE",
    "AllenCahnPDE",
    "KPZInterfacePDE",
    "KleinGordonPDE",
    "KuramotoSivashinskyPDE",
    "SwiftHohenbergPDE",
    "WavePDE",
    "BoundariesList",
    "CahnHilliardPDE",
    "CartesianGrid",
    "Controller",
    "ConvergenceError",
    "CrankNicolsonSolver",
    "DiffusionPDE",
    "EulerSolver",
    "FieldCollection",
    "ExplicitSolver",
    "FieldDomains",
    "FieldHistogram",
    "FieldSpectrum",
    "FieldStatistics",
    "HipBackend",
    "ImplicitSolver",
    "RungeKuttaSolver",
    "ScalarField",
    "Tensor2Field",
    "UnitGrid",
    "VectorField",
    "field_domains",
    "domain_properties",
    "field_histogram",
    "field_median",
    "field_quantile",
    "field_spectrum",
    "field_statistics",
    "get_backend",
    "image_data",
    "interpolate_to_grid",
    "line_data",
    "project",
    "slice_field",
    "smooth",
    "solve_laplace_equation",
    "solve_poisson_equation",
]
__version__ = "0.1.0"
