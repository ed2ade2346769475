"""State residency between the calls of a stepper: :class:`ResidentState` and the field class that pulls the device copy on host access.  Split from
``backend.py`` in round 6 (no behaviour change).

Also what the device-side analysis of a resident state shares (``statistics.py``, ``distribution.py``, ``domains.py``, ``projection.py``,
``smoothing.py``, ``interpolation.py``): the access to a field's link and its two predicates (:func:`link_of`, :func:`resident_link`,
:func:`valid_link`), the helpers :func:`backend_of`, :func:`is_collection`, :func:`base_class` and :func:`field_dtype`, the boolean
opt-in of a backend (:class:`DeviceOption`) and the opening of a call that reads the device copy (:func:`device_source`).
"""

from __future__ import annotations

import contextlib
import logging

import numpy as np

from .device import DeviceArray

_logger = logging.getLogger("pde_hip.backend")


def _config_get(config, key: str, default):
    try:
        if config is not None and key in config:
            return config[key]
    except TypeError:
        pass
    return default


_DATA_ATTRIBUTES = frozenset({"data", "_data_valid", "_data_full", "_FieldBase__data_full"})
_STATISTICS_ATTRIBUTES = frozenset({"integral", "average", "fluctuations", "magnitude", "integrals", "averages", "magnitudes"})
_PROJECTION_METHODS = frozenset({"project", "slice", "get_line_data", "get_image_data"})
_SMOOTHING_METHODS = frozenset({"smooth"})
_SYNCED_CLASSES: dict[type, type] = {}


def link_of(obj):
    """The :class:`ResidentState` that ``obj`` carries, whatever its state, else None (bare arrays, host fields, copies of fields)."""
    return getattr(obj, "__dict__", {}).get("_hip_link")


def resident_link(obj):
    """The :class:`ResidentState` of a field whose DEVICE copy is AHEAD (:attr:`ResidentState.device_ahead`), else None."""
    link = link_of(obj)
    return link if link is not None and link.device_ahead else None


def valid_link(obj):
    """The :class:`ResidentState` of a field whose device copy is VALID (:attr:`ResidentState.device_valid`), else None."""
    link = link_of(obj)
    return link if link is not None and link.device_valid else None


def base_class(obj) -> type:
    """The field's own class (``type(obj)`` of a resident field is the intercepting subclass)."""
    return getattr(type(obj), "_hip_base_class", type(obj))


def is_collection(obj) -> bool:
    return getattr(obj, "fields", None) is not None or getattr(obj, "_fields", None) is not None


def field_dtype(field) -> np.dtype:
    """The type of the field's data without touching ``field.data`` (py-pde's ``dtype`` reads ``_data_full``: a resident state would
    come down).  A field with a link has the type of the link's device array in every state: the link is made from the field's type
    and the ``data`` setters write into the existing arrays.  (Only py-pde's private ``_data_full = array_of_another_type`` on a field
    whose host copy is current could part the two; the next stepper call converts such data to the device array's type anyway.)"""
    link = link_of(field)
    return np.dtype(link.dev_state.host_dtype if link is not None else field.dtype)


def backend_of(obj, backend):
    """The backend that serves a module-level call: that of the object's link, else ``backend`` itself, else the backend of that name
    of py-pde (for its fields; a collection is judged by its first field) or of this package."""
    link = link_of(obj)
    if link is not None:
        return link.backend
    if not isinstance(backend, str):
        return backend
    probe = next(iter(obj), obj) if is_collection(obj) else obj
    if type(probe).__module__.split(".")[0] == "pde":
        from pde.backends import get_backend as pde_get_backend

        from . import pypde_plugin  # noqa: F401  (registers "hip")

        return pde_get_backend(backend)
    from .backend import get_backend

    return get_backend(backend)


def kernels_take(backend, dev: DeviceArray, needs, max_comp: int | None = 64) -> bool:
    """Real components (no planar complex pairs), at most ``max_comp`` of them, and a library that has the entry points ``needs``."""
    return not dev.complex_pairs and (max_comp is None or dev.ncomp <= max_comp) and backend._lib.has(*needs)


def device_source(backend, obj, *, needs, max_comp: int | None = 64):
    """``(device array or None, bare)``: how a call that reads a state where it lives opens.  ``bare``: ``obj`` is a
    :class:`DeviceArray` itself; else the device array is that of a field whose device copy is ahead (:func:`resident_link`).  None where
    there is no such array or the kernels do not take it (:func:`kernels_take`): the caller's host path.  What one feature refuses
    beyond that (collections, ranks, component shapes) is that feature's business."""
    bare = isinstance(obj, DeviceArray)
    link = None if bare else resident_link(obj)
    dev = obj if bare else (link.dev_state if link is not None else None)
    if dev is not None and not kernels_take(backend, dev, needs, max_comp):
        dev = None
    return dev, bare


class DeviceOption:
    """A boolean opt-in of the backend: the value set on the instance, else ``config[name]``, else False; setting None clears the
    instance's value, so that the configuration decides again."""

    def __init__(self, doc: str):
        self.__doc__ = doc

    def __set_name__(self, owner, name: str) -> None:
        self.name = name

    def __get__(self, backend, owner=None):
        if backend is None:
            return self
        value = getattr(backend, "_" + self.name, None)
        if value is not None:
            return value
        try:
            if self.name in backend.config:
                return bool(backend.config[self.name])
        except TypeError:
            pass
        return False

    def __set__(self, backend, value) -> None:
        setattr(backend, "_" + self.name, None if value is None else bool(value))


class ResidentState:
    """Link between a host field object and its device-resident copy (no full-field PCIe traffic per
    tracker interrupt; reference behaviour being replaced: ``pde/backends/torch/backend.py:654-662``).

    The field object handed to the stepper keeps its identity (the controller returns it, trackers receive it), but its
    class is swapped for a dynamic subclass whose data attributes (``data``, ``_data_full`` ...) first bring the host
    arrays up to date — one pinned-speed download — and then count as a possible modification, so the next stepper call
    uploads again.  Nothing else about the field changes; copies of it are ordinary fields.

    Limitation: synchronisation happens on ATTRIBUTE ACCESS.  A numpy view obtained earlier (``arr = state.data``
    kept by a tracker or by the caller) is not refreshed behind the holder's back while the run goes on — it shows the state of
    its last ``state.data`` access — and writes made through such a held view after that access are not seen.  Code that wants
    the reference's behaviour (the stepper updates the host array in place at every call) sets ``resident_state=False`` in the
    backend's configuration, which restores the upload / download per stepper call of ``pde/backends/torch/backend.py:654-662``.

    ``(host_stale, host_touched)`` has three reachable states (a stepper pushes before the device advances, and a host access pulls
    before it counts as a modification, so both are never set together):

    * ``(False, True)``  the HOST copy is the current one: before the first upload, and from the first host access after a stepper call;
    * ``(False, False)`` both copies are EQUAL: after an upload, before the device advanced;
    * ``(True, False)``  the DEVICE copy is ahead: between a stepper call and the next host access.

    Two questions are asked of them.  :attr:`device_ahead`: the reductions (statistics, histograms, domains, projections, smoothing,
    the finiteness check) read the device copy only while it is AHEAD - with both copies equal they answer from the host, where they
    give numpy's bits.  :attr:`device_valid`: interpolation reads the device copy whenever it is VALID, equal or ahead - its kernels
    restate the host arithmetic operation by operation, so nothing is gained by going back to the host.
    """

    def __init__(self, field, dev_state: DeviceArray, backend):
        self.dev_state, self.backend = dev_state, backend
        self.host_stale = False          # device is ahead of the host arrays
        self.host_touched = True         # host arrays may differ from the device copy (initially: never uploaded)
        self.downloads = self.uploads = 0

    @property
    def device_ahead(self) -> bool:
        """The device copy is ahead of the host arrays (``host_stale``)."""
        return self.host_stale

    @property
    def device_valid(self) -> bool:
        """The device copy holds the current state: equal to the host arrays, or ahead of them (``not host_touched``)."""
        return not self.host_touched

    @staticmethod
    @contextlib.contextmanager
    def plain_access(field, write: bool = False):
        """``field.data`` as plain host memory inside the block: the interception of a resident field is off meanwhile.  ``write``: the
        block wrote the host arrays, so the next stepper call uploads them."""
        link = link_of(field)
        if link is None:
            yield
            return
        field.__dict__["_hip_link"] = None
        try:
            yield
        finally:
            field.__dict__["_hip_link"] = link
        if write:
            link.host_touched = True

    @staticmethod
    def attach(field, dev_state: DeviceArray, backend) -> "ResidentState":
        link = link_of(field)
        cls = type(field)
        base = getattr(cls, "_hip_base_class", cls)
        if base not in _SYNCED_CLASSES:
            _SYNCED_CLASSES[base] = _make_synced_class(base)
        if link is not None and link.dev_state is dev_state:
            if cls is base:              # a host access since the last call put the plain class back (before_host_access)
                field.__class__ = _SYNCED_CLASSES[base]
            return link
        if link is not None:             # a stepper of an earlier run: settle it first
            link.pull(field)
        link = ResidentState(field, dev_state, backend)
        field.__dict__["_hip_link"] = link
        link._field_ref = field
        if cls is base:
            field.__class__ = _SYNCED_CLASSES[base]
        return link

    def __reduce__(self):
        # a field that was read after the run is a plain py-pde object again but still carries this link in its `__dict__` (the next
        # stepper call picks it up): copies and pickles of the field get `None` in its place
        return (type(None), ())

    def __deepcopy__(self, memo):
        return None

    def _host_valid(self):
        field = self._field_ref
        base = getattr(type(field), "_hip_base_class", type(field))
        return base.data.fget(field) if isinstance(getattr(base, "data", None), property) else object.__getattribute__(field, "data")

    def push(self) -> None:
        if self.host_touched:
            field = self._field_ref
            with self.plain_access(field):
                self.dev_state.set_valid(field.data, self.backend.stream)
            self.host_touched, self.host_stale = False, False
            self.uploads += 1

    def device_advanced(self) -> None:
        self.host_stale = True

    def pull(self, field=None) -> None:
        """Bring the host arrays up to date (called on the first data access after the device advanced)."""
        field = self._field_ref if field is None else field
        if self.host_stale:
            self.host_stale = False
            with self.plain_access(field):
                self.dev_state.get_valid(out=field.data, stream=self.backend.stream)
            self.downloads += 1

    def before_host_access(self) -> None:
        """First access to the data after a stepper call: the host arrays are current from here on and may be written, so nothing
        needs intercepting until the next stepper call - the field gets its own class back (``type(result) is pde.ScalarField`` once
        the result has been looked at; `attach` swaps the intercepting subclass in again)."""
        self.pull()
        self.host_touched = True
        field = self._field_ref
        base = getattr(type(field), "_hip_base_class", None)
        if base is not None:
            object.__dict__["__class__"].__set__(field, base)


def _device_statistic(link, field, name: str):
    from .statistics import NOT_ANSWERED, device_property

    value = device_property(link, field, name)
    return value is not NOT_ANSWERED, value


def _device_projection(link, field, name: str):
    from .projection import device_method

    method = device_method(link, field, name)
    return method is not None, method


def _device_smoothing(link, field, name: str):
    from .smoothing import device_method

    method = device_method(link, field, name)
    return method is not None, method


# The opt-ins (default off), in the order they are asked: (attributes, option of the backend, answer -> (answered, value)).  While the
# device copy is ahead and the option is on, the attribute is answered from the device copy - no download, and the class stays swapped
# in.  Whatever the device path does not take falls through to the reference's attribute, which reads `data`.
_OPT_INS = (
    # `integral`, `average`, `fluctuations`, `magnitude` and the collection's plurals
    (_STATISTICS_ATTRIBUTES, "device_statistics", _device_statistic),
    # projections, slices and the data behind line and image plots of a real scalar field
    (_PROJECTION_METHODS, "device_projections", _device_projection),
    # `smooth` of a real field runs on the device copy; only a host result comes down
    (_SMOOTHING_METHODS, "device_smoothing", _device_smoothing),
)


def _make_synced_class(base: type) -> type:
    def __getattribute__(self, name):
        for names, option, answer in _OPT_INS:
            if name in names:
                link = object.__getattribute__(self, "__dict__").get("_hip_link")
                if link is not None and link.host_stale and getattr(link.backend, option, False):
                    answered, value = answer(link, self, name)
                    if answered:
                        return value
        if name in _DATA_ATTRIBUTES:
            link = object.__getattribute__(self, "__dict__").get("_hip_link")
            if link is not None:
                link.before_host_access()
        return base.__getattribute__(self, name)

    def __reduce_ex__(self, protocol):
        # pickling / deepcopy: settle the data and present the plain class, without the link
        link = link_of(self)
        if link is not None:
            link.pull(self)
        self.__dict__.pop("_hip_link", None)
        self.__class__ = base
        return base.__reduce_ex__(self, protocol)

    # `field.__class__` keeps answering with the field's own class: py-pde compares classes by identity before any binary
    # operation (`assert_field_compatible`, pde/fields/base.py:385-390) and builds copies from `self.__class__`; only
    # `type(field)` shows the intercepting subclass
    real_class = object.__dict__["__class__"]

    def _get_class(self):
        return base

    def _set_class(self, value):
        real_class.__set__(self, value)

    # py-pde registers every field subclass by NAME (pde/fields/base.py:77-88) to rebuild fields from stored attributes: the
    # registry must keep pointing at the real class
    import warnings

    registry = getattr(base, "_subclasses", None)
    previous = registry.get(base.__name__) if isinstance(registry, dict) else None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        synced = type(base.__name__, (base,), {"__getattribute__": __getattribute__, "__reduce_ex__": __reduce_ex__, "_hip_base_class": base,
                                               "__class__": property(_get_class, _set_class),
                                               "__module__": base.__module__, "__qualname__": base.__qualname__, "__doc__": base.__doc__})
    if previous is not None:
        registry[base.__name__] = previous
    return synced
