"""What the device-side analysis features share in ``pde_hip/resident.py``: the two predicates of a field's link, the opening
``device_source`` of a call that reads the device copy, and the boolean opt-in of the backend.  No GPU and no library: stand-ins only.

The expected values are those of the call sites these helpers were taken from (``make_statistics``, ``SteadyStateCheck._device_state``,
``_distribution_source``, ``projection.device_copy``, ``interpolation``'s link rule), written down from that code."""

from __future__ import annotations

import itertools

import pytest

from pde_hip.device import DeviceArray
from pde_hip.resident import DeviceOption, device_source, kernels_take, link_of, resident_link, valid_link

# (host_stale, host_touched) -> name; (True, True) is not reachable
HOST_CURRENT, EQUAL, DEVICE_AHEAD = (False, True), (False, False), (True, False)
STATES = {"host_current": HOST_CURRENT, "equal": EQUAL, "device_ahead": DEVICE_AHEAD}


class FakeArray(DeviceArray):
    """A device array that is nothing but the three attributes the opening reads."""

    def __init__(self, comp_shape=(), complex_pairs=False):
        self.comp_shape, self.complex_pairs = tuple(comp_shape), bool(complex_pairs)
        self.ncomp = 1
        for c in self.comp_shape:
            self.ncomp *= c


class FakeLib:
    def __init__(self, *entries):
        self.entries = set(entries)

    def has(self, *names) -> bool:
        return all(n in self.entries for n in names)


class FakeBackend:
    def __init__(self, *entries):
        self._lib = FakeLib(*entries)


class FakeLink:
    def __init__(self, state, dev, backend=None):
        self.host_stale, self.host_touched = state
        self.dev_state, self.backend = dev, backend

    # the two predicates are those of ResidentState itself
    from pde_hip.resident import ResidentState as _R

    device_ahead = _R.device_ahead
    device_valid = _R.device_valid


class FakeField:
    rank = 0

    def __init__(self, link=None, rank=0):
        self.rank = rank
        if link is not None:
            self.__dict__["_hip_link"] = link


class FakeCollection(FakeField):
    def __init__(self, link=None):
        super().__init__(link)
        self.fields = [FakeField(), FakeField()]

    def __iter__(self):
        return iter(self.fields)


NEEDS = ("alpha", "beta")


@pytest.mark.parametrize("name", sorted(STATES))
def test_predicates_in_the_three_reachable_states(name):
    link = FakeLink(STATES[name], FakeArray())
    field = FakeField(link)
    assert link_of(field) is link
    # the reductions: only while the device copy is AHEAD (`host_stale`)
    assert (resident_link(field) is link) == (name == "device_ahead")
    # interpolation: whenever the device copy is VALID (`not host_touched`)
    assert (valid_link(field) is link) == (name in ("equal", "device_ahead"))
    assert link.device_ahead == (name == "device_ahead") and link.device_valid == (name != "host_current")


def test_objects_without_a_link():
    for obj in (FakeField(), FakeArray(), object(), 3.0):
        assert link_of(obj) is None and resident_link(obj) is None and valid_link(obj) is None


# ---- device_source: every combination, the expectation spelled as the call sites spelled it ---------------------------------------------
KINDS = ("bare", "resident", "host", "collection")
CASES = list(itertools.product(KINDS, sorted(STATES), (False, True), (64, 65), (True, False), (64, None)))


@pytest.mark.parametrize(("kind", "state", "cplx", "ncomp", "present", "max_comp"), CASES)
def test_device_source(kind, state, cplx, ncomp, present, max_comp):
    # 64 components: (64,); 65: (65,); complex pairs carry a trailing axis of 2, so 64 -> (32, 2) and 65 -> (33, 2) = 66 > 64
    dev = FakeArray((32 if ncomp == 64 else 33, 2) if cplx else (ncomp,), complex_pairs=cplx)
    backend = FakeBackend(*(NEEDS if present else NEEDS[:1]))
    link = FakeLink(STATES[state], dev, backend)
    obj = {"bare": dev, "resident": FakeField(link), "host": FakeField(), "collection": FakeCollection(link)}[kind]
    got, bare = device_source(backend, obj, needs=NEEDS, max_comp=max_comp)

    # steps 1 and 2: a bare array is read as it is; a field (a collection too: `make_statistics` asks nothing else) only while its
    # device copy is ahead; a host field never
    reached = kind == "bare" or (kind in ("resident", "collection") and state == "device_ahead")
    # step 3: real components, at most `max_comp` of them (`make_statistics` sets no limit here), every entry point present
    taken = not cplx and (max_comp is None or dev.ncomp <= max_comp) and present
    assert bare == (kind == "bare")
    assert got is (dev if reached and taken else None)
    assert kernels_take(backend, dev, NEEDS, max_comp) == taken


def test_what_stays_with_the_features():
    """The refusals of one feature are not in the opening: a collection whose device copy is ahead is a source for the statistics, the
    histogram takes the host path for it, and projections take real scalar fields only."""
    from pde_hip.distribution import DistributionMixin
    from pde_hip.projection import device_copy

    backend = FakeBackend("histogram", "quantile_select", "field_stats", "steady_state", "project", "extract_box")
    scalar, vector = FakeArray(()), FakeArray((3,))
    coll = FakeCollection(FakeLink(DEVICE_AHEAD, vector, backend))
    assert device_source(backend, coll, needs=("field_stats", "steady_state"), max_comp=None) == (vector, False)
    dev, host = DistributionMixin._distribution_source(backend, coll, None)
    assert dev is None and callable(host)
    assert DistributionMixin._distribution_source(backend, FakeField(FakeLink(DEVICE_AHEAD, vector, backend)), None) == (vector, None)
    assert DistributionMixin._distribution_source(backend, FakeArray((65,)), None)[0] is None

    assert device_copy(backend, coll) is None
    assert device_copy(backend, FakeField(FakeLink(DEVICE_AHEAD, scalar, backend))) is scalar
    assert device_copy(backend, FakeField(FakeLink(EQUAL, scalar, backend))) is None
    assert device_copy(backend, FakeField(FakeLink(DEVICE_AHEAD, vector, backend), rank=1)) is None
    assert device_copy(backend, FakeField(FakeLink(DEVICE_AHEAD, vector, backend))) is None          # (rank 0 over a vector state)
    assert device_copy(backend, vector) is vector and device_copy(backend, FakeArray((65,))) is None
    assert device_copy(backend, FakeArray((2,), complex_pairs=True)) is None
    assert device_copy(FakeBackend("project"), scalar) is None


def test_steady_state_check_learns_its_backend_from_the_state():
    from pde_hip.statistics import SteadyStateCheck

    backend = FakeBackend("field_stats", "steady_state")
    dev = FakeArray((2,))
    check = SteadyStateCheck(None)
    assert check._device_state(dev) is None and check.backend is None                      # a bare array brings no backend
    assert check._device_state(FakeField(FakeLink(EQUAL, dev, backend))) is None and check.backend is None
    assert check._device_state(FakeField(FakeLink(DEVICE_AHEAD, dev, backend))) is dev and check.backend is backend
    assert check._device_state(dev) is dev
    other = FakeBackend()
    assert SteadyStateCheck(other)._device_state(FakeField(FakeLink(DEVICE_AHEAD, dev, backend))) is None      # its own backend decides


# ---- the opt-in --------------------------------------------------------------------------------------------------------------------------
class _Backend:
    device_things = DeviceOption("""Whether things happen on the device.""")

    def __init__(self, config):
        self.config = config


def test_option_resolves_override_then_config_then_false():
    assert _Backend.device_things.__doc__ == "Whether things happen on the device."
    assert _Backend({}).device_things is False
    assert _Backend(None).device_things is False                      # (a backend without a configuration)
    assert _Backend({"device_things": 1}).device_things is True
    assert _Backend({"device_things": 0}).device_things is False
    b = _Backend({"device_things": True})
    b.device_things = False
    assert b.device_things is False                                    # the override wins
    b.device_things = None
    assert b.device_things is True                                     # None clears it: the configuration decides again
    b = _Backend({})
    b.device_things = "yes"
    assert b.device_things is True
    b.device_things = None
    assert b.device_things is False


def test_the_three_options_of_the_backend_are_such_options():
    from pde_hip.projection import ProjectionMixin
    from pde_hip.smoothing import SmoothingMixin
    from pde_hip.statistics import StatisticsMixin

    for cls, name in ((StatisticsMixin, "device_statistics"), (ProjectionMixin, "device_projections"), (SmoothingMixin, "device_smoothing")):
        option = getattr(cls, name)
        assert isinstance(option, DeviceOption) and option.name == name and f"backend.hip.{name}" in option.__doc__
