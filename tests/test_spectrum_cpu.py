"""The spectrum without a GPU: the serial C versions of the tests-only shim (tests/shim/pdehip_shim_spectrum.c) against numpy, and
``pde_hip.field_spectrum`` through the shim and on the host path.

Bounds: ``tests/spectrum_cases.py`` (Higham's bound for the transform, the limb layout for the sums, Cauchy-Schwarz for the shell sums
against numpy).  Observed ratios: ``profiles/spectrum_tests.md``.  The device kernels are compared with the shim bit by bit in
``tests/test_hip_spectrum.py``.
"""

from __future__ import annotations

import math
from pathlib import Path

import numpy as np
import pytest
import shimlib
import spectrum_cases as K
import spectrum_shimlib
import stats_shimlib

import pde_hip
from pde_hip import _abi
from pde_hip.device import DeviceArray
from pde_hip.spectrum import FieldSpectrum, default_edges, shell_edges

IDS = ["f64", "f32"]
GOLDEN = Path(__file__).resolve().parent / "golden" / "spectrum.npz"


@pytest.fixture
def shim():
    with spectrum_shimlib.use_shim() as lib:
        yield lib


def test_abi_table():
    names = {"fft_supported", "fft_forward", "shell_spectrum"}
    assert _abi.ABI_VERSION == 8 and names <= set(_abi.OPTIONAL_PROTOTYPES)
    assert not names & (set(_abi.COMPUTE_PROTOTYPES) | set(_abi.COMM_PROTOTYPES) | set(_abi.RUNTIME_PROTOTYPES))
    for module in (shimlib, stats_shimlib):
        with module.use_shim() as lib:
            assert not lib.has("fft_supported") and not lib.has("shell_spectrum")
    with spectrum_shimlib.use_shim() as lib:
        assert lib.has("fft_supported", "fft_forward", "shell_spectrum")
    assert {"field_spectrum", "FieldSpectrum"} <= set(pde_hip.__all__)


# ---- the transform ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_shim_transform_against_numpy(shape, dtype):
    valid = K.inputs(shape, 3, np.dtype(dtype).name)
    got = K.shim_forward(shape, 3, np.dtype(dtype).name)
    expect = np.fft.rfftn(valid.astype(np.float64), axes=tuple(range(1, valid.ndim)))
    assert got.shape == expect.shape
    for c in range(3):
        err, norm = np.linalg.norm((got[c] - expect[c]).ravel()), np.linalg.norm(expect[c].ravel())
        print(f"{K.shape_id(shape)} c{c}: error / bound = {err / (K.transform_eps(shape) * norm):.4f}")
        assert err <= K.transform_eps(shape) * norm


def test_dry_run_refuses_what_the_transform_does_not_take():
    sh = K.shim()
    for shape in K.SHAPES + (K.TURN, (1,), (1, 8), (1024, 1024, 4096)):
        assert sh.supported(shape) == 0 and sh.supported(shape, np.float32) == 0, shape
    for shape in K.REFUSED:
        assert sh.supported(shape) == 2, shape


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("default", "seven", "explicit"))
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_shim_counts_equal_numpys_histogram_of_the_full_grid(shape, which):
    edges = K.edge_sets(shape)[which]
    counts, _ = K.shim_shells(shape, 3, "float64", which)
    expect = K.np_counts(shape, edges)
    np.testing.assert_array_equal(counts, expect)
    assert int(counts.sum()) == math.prod(shape)
    if which == "default":
        assert counts[0] == 1 and counts[-2] == 0 and counts[-1] == 0
    if which == "explicit" and math.prod(shape) > 64:
        assert counts[-2] > 0 and counts[-1] > 0          # modes below and above the edges


# ---- sums ------------------------------------------------------------------------------------------------------------------------------
def test_limb_bound_is_below_two_ulp_for_every_supported_shape():
    """A shell holds at most 2**32 modes.  Whatever the largest term and the sum (>= the largest term), the bound stays below 2 ulp."""
    for L in range(33):
        count = 1 << L
        for largest in (1.0, 1.0 - 2.0 ** -53, 3e-200, 7e250):
            for total in (largest, largest * min(count, 2.0 ** 20)):
                assert K.limb_bound(largest, count, total) < 2.0 * K.ulp(total), (L, largest, total)
                eh, l, d, el = K.limb_layout(largest, count)
                assert l == L and largest < 2.0 ** (eh + 62 - L) and count * 2.0 ** (62 - L) <= 2.0 ** 62


@pytest.mark.parametrize("dtype", K.DTYPES, ids=IDS)
@pytest.mark.parametrize("which", ("default", "seven", "explicit"))
@pytest.mark.parametrize("shape", K.SHAPES, ids=K.shape_id)
def test_shim_sums(shape, which, dtype):
    name = np.dtype(dtype).name
    edges = K.edge_sets(shape)[which]
    valid, spec = K.inputs(shape, 3, name), K.shim_forward(shape, 3, name)
    counts, sums = K.shim_shells(shape, 3, name, which)
    slot, weight = K.half_slots(shape, edges)
    terms = K.weighted_power(spec, weight)
    exact = K.exact_shell_sums(terms, slot, len(edges) + 1)
    worst = 0.0
    for c in range(3):
        for b in range(len(edges) + 1):
            mine = terms[c][slot == b]
            bound = K.limb_bound(float(mine.max()) if mine.size else 0.0, int(counts[b]), exact[c, b])
            assert abs(sums[c, b] - exact[c, b]) <= bound, (c, b, sums[c, b], exact[c, b], bound)
            if exact[c, b]:
                worst = max(worst, abs(sums[c, b] - exact[c, b]) / K.ulp(exact[c, b]))
    eps = K.transform_eps(shape)
    reference = K.np_shell_sums(shape, valid, edges)
    ratio = np.abs(sums - reference).sum(axis=1) / (eps * (2.0 + eps) * reference.sum(axis=1))
    print(f"{K.shape_id(shape)} {which}: limbs off by {worst:.2f} ulp at most; against numpy / bound = {ratio.max():.4f}")
    assert (ratio <= 1.0).all()
    again = K.shim().shells(shape, valid, K.frequencies(shape), edges)
    np.testing.assert_array_equal(K.bits(again[1]), K.bits(sums))


def test_shell_without_finite_maximum_reports_it():
    shape = (8, 8)
    valid = np.array(K.inputs(shape, 1, "float64"))
    valid[0, 3, 3] = np.inf
    counts, sums = K.shim().shells(shape, valid, K.frequencies(shape), K.edge_sets(shape)["default"])
    assert int(counts.sum()) == 64 and not np.isfinite(sums[0, :-2]).any()


# ---- structure: sums of cosines of integer amplitude ------------------------------------------------------------------------------------------
STRUCTURE = (
    ((64,), (1.0,), ((3, (5,)),)),
    ((32, 64), (2.0, 1.0), ((2, (3, 0)), (1, (0, 17)))),
    ((16, 16, 32), (2.0, 2.0, 1.0), ((4, (0, 0, 6)), (1, (2, 1, 0)))),
)


@pytest.mark.parametrize("case", STRUCTURE, ids=lambda c: K.shape_id(c[0]))
def test_structure_of_cosine_fields(shim, case):
    """Every axis has the same length L = n dx, so dk = 1 / L and the mode m lies at |m| / L: in the shell round(|m|) of the default
    shells.  A cosine of amplitude a puts a**2 / 4 / prod(dx) into each of +m and -m."""
    shape, dx, modes = case
    backend = pde_hip.get_backend("hip")
    length = shape[0] * dx[0]
    assert all(n * d == length for n, d in zip(shape, dx))
    data = K.cosine_field(shape, modes)
    dev = DeviceArray(backend.grid_info(pde_hip.CartesianGrid([[0, length]] * len(shape), shape, periodic=True), np.float64), ()).set_valid(data)
    got = pde_hip.field_spectrum(dev, backend=backend)
    assert got.on_device and got.counts[0] == 1 and int(got.counts.sum()) == data.size
    eps = K.transform_eps(shape)
    total = sum(a * a / 2.0 for a, _ in modes) / math.prod(dx)
    shells = sorted({round(math.sqrt(sum(mi * mi for mi in m))) for _, m in modes})
    outside = np.delete(got.power, shells).sum()
    print(f"power outside the modes' shells / bound = {outside / (eps * (2 + eps) * total):.3e}")
    assert outside <= eps * (2.0 + eps) * total
    strongest = max(modes, key=lambda am: am[0])
    k_strongest = math.sqrt(sum(mi * mi for mi in strongest[1])) / length
    if float(k_strongest * length).is_integer():
        assert got.k_peak == k_strongest
    # Parseval: total * prod(dx) is the mean square of the field
    assert abs(got.total * math.prod(dx) - np.mean(data * data)) <= (eps * (2.0 + eps) + 4 * K.U) * np.mean(data * data)
    inside = got.power[shells]
    k_mean = (got.k[shells] * inside).sum() / inside.sum()
    assert abs(got.mean_wavenumber - k_mean) <= 4.0 * eps * k_mean and abs(got.length_scale * got.mean_wavenumber - 1.0) <= 4 * K.U


# ---- the golden file: the reference's own spectral_density --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.GOLDEN))
def test_golden(shim, name):
    backend = pde_hip.get_backend("hip")
    gold = np.load(GOLDEN)
    shape, dx = K.GOLDEN[name]
    data, kk, density = gold[f"{name}/data"], gold[f"{name}/k"], gold[f"{name}/density"]
    np.testing.assert_array_equal(data, K.golden_input(name))
    np.testing.assert_array_equal(gold[f"{name}/dx"], dx)
    grid = pde_hip.CartesianGrid([[0, n * d] for n, d in zip(shape, dx)], shape, periodic=True)
    eps = K.transform_eps(shape)
    power_of_two = all(n & (n - 1) == 0 for n in shape)
    dev = DeviceArray(backend.grid_info(grid, np.float64), ()).set_valid(data)
    host = backend.make_spectrum(grid)
    for bins in (None, 5, np.array([0.05, 0.2, 0.21, 0.5]) * kk.max()):
        results = {"device array": pde_hip.field_spectrum(dev, bins, backend=backend), "host": host(data, bins)}
        assert results["device array"].on_device == power_of_two and not results["host"].on_device
        for what, got in results.items():
            # the reference's |k| decides the shell of every mode, its density is summed per shell
            np.testing.assert_array_equal(got.counts, np.histogram(kk.ravel(), got.edges)[0], err_msg=what)
            expect = np.histogram(kk.ravel(), got.edges, weights=density.ravel())[0]
            assert got.below.counts == np.count_nonzero(kk < got.edges[0]) and got.above.counts == np.count_nonzero(kk > got.edges[-1])
            assert np.abs(got.power - expect).sum() <= eps * (2.0 + eps) * density.sum(), what
            everything = got.total
            assert abs(everything - density.sum()) <= eps * (2.0 + eps) * density.sum()
            with np.errstate(invalid="ignore", divide="ignore"):
                np.testing.assert_array_equal(got.density, np.where(got.counts > 0, got.power / got.counts, np.nan))


# ---- the interface ---------------------------------------------------------------------------------------------------------------------
def test_default_shells_and_their_limits():
    edges, centres = default_edges((64, 32), (0.5, 1.0))
    dk = 1.0 / 32.0
    assert edges[0] == 0.0 and edges[1] == 0.5 * dk and centres[0] == 0.0 and centres[3] == 3 * dk
    assert edges[-1] >= K.full_k((64, 32), (0.5, 1.0)).max() > edges[-2]
    with pytest.raises(ValueError, match="explicit edges"):
        default_edges((4096 * 4,), (1.0,))          # 8193 shells
    with pytest.raises(ValueError, match="explicit edges"):
        default_edges((2, 4096), (4096.0, 0.5))      # dk from the long axis, |k| from the short spacing
    for bad in ("auto", 0, 4097, [1.0], [0.0, 0.0, 1.0], [0.0, np.nan], 2.5):
        with pytest.raises(ValueError):
            shell_edges(bad, (8, 8), (1.0, 1.0))
    assert shell_edges(4, (8, 8), (1.0, 1.0))[0].size == 5


def test_zero_mode_rules(shim):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([16, 16], periodic=True)
    data = K.cosine_field((16, 16), ((2, (3, 0)),)) + 5.0
    spectrum = backend.make_spectrum(grid)
    default = spectrum(data)
    assert isinstance(default, FieldSpectrum) and not default.on_device and default.k_peak == 3.0 / 16.0
    assert abs(default.length_scale - 16.0 / 3.0) < 1e-9          # (the mean of 5 does not enter)
    positive = spectrum(data, [0.01, 0.1, 0.3, 0.8])
    assert abs(positive.mean_wavenumber - 0.2) < 1e-9
    for bins in (4, [0.0, 0.1, 0.8]):
        got = spectrum(data, bins)
        for name in ("k_peak", "mean_wavenumber", "length_scale"):
            with pytest.raises(ValueError, match="zero mode"):
                getattr(got, name)
    empty = spectrum(data, [0.001, 0.002, 0.003])
    assert np.isnan(empty.density).all() and (empty.counts == 0).all()


def test_components_and_bare_arrays(shim):
    """A vector field: one set of shells, power per component; the device array and the host array of the same data agree within the
    transform bound, an fp32 array is converted exactly."""
    backend = pde_hip.get_backend("hip")
    shape = (16, 4, 128)
    grid = pde_hip.CartesianGrid([[0, n * d] for n, d in zip(shape, K.DX)], shape, periodic=True)
    for dtype in K.DTYPES:
        data = K.inputs(shape, 3, np.dtype(dtype).name)
        dev = DeviceArray(backend.grid_info(grid, dtype), (3,)).set_valid(data)
        on_device, on_host = pde_hip.field_spectrum(dev, backend=backend), backend.make_spectrum(grid)(data)
        assert on_device.on_device and not on_host.on_device and on_device.power.shape == (3, on_device.counts.size)
        np.testing.assert_array_equal(on_device.counts, on_host.counts)
        np.testing.assert_array_equal(on_device.edges, on_host.edges)
        eps = K.transform_eps(shape)
        assert (np.abs(on_device.power - on_host.power).sum(axis=1) <= eps * (2.0 + eps) * on_host.power.sum(axis=1)).all()
        assert on_device.k_peak.shape == (3,) and on_device.length_scale.shape == (3,)
    with pytest.raises(ValueError, match="make_spectrum"):
        backend.make_spectrum()(np.zeros((4, 4)))


def test_a_refused_shape_takes_the_host_path(shim):
    backend = pde_hip.get_backend("hip")
    for shape in ((12, 10), (2048, 8)):
        grid = pde_hip.UnitGrid(shape, periodic=True)
        data = np.random.default_rng(2).normal(size=shape)
        dev = DeviceArray(backend.grid_info(grid, np.float64), ()).set_valid(data)
        got = pde_hip.field_spectrum(dev, backend=backend)
        assert not got.on_device and int(got.counts.sum()) == data.size
        assert abs(got.total - np.mean(data * data)) <= 1e-12 * np.mean(data * data)


def test_refusals_by_name(shim):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([8, 8], periodic=True)
    fields = [pde_hip.ScalarField(grid, np.ones((8, 8))), pde_hip.ScalarField(grid, np.ones((8, 8)))]
    with pytest.raises(TypeError, match="collection"):
        pde_hip.field_spectrum(pde_hip.FieldCollection(fields), backend=backend)

    class PolarGrid:
        shape, discretization, periodic, dim = (8,), (1.0,), (False,), 2

    class Disk:
        grid, data = PolarGrid(), np.ones(8)

    with pytest.raises(TypeError, match="PolarGrid"):
        backend.make_spectrum()(Disk())


# ---- residency -------------------------------------------------------------------------------------------------------------------------
class _FakeInfo:
    shape, dx, ref = (8, 16), (1.0, 1.0), None


class _FakeArray(DeviceArray):
    """A device array that is nothing but what the opening of a spectrum call reads (tests/test_resident_source.py's style)."""

    def __init__(self, data, complex_pairs=False):
        self.data, self.info, self.comp_shape, self.ncomp, self.complex_pairs = data, _FakeInfo(), (), 1, complex_pairs


class _FakeLib:
    def __init__(self, entries, refuse):
        self.entries, self.refuse = set(entries), refuse

    def has(self, *names):
        return all(n in self.entries for n in names)

    def fft_supported(self, ref):
        if self.refuse:
            raise NotImplementedError("fft: axis 0 has 12 cells")


class _FakeLink:
    from pde_hip.resident import ResidentState as _R

    device_ahead, device_valid = _R.device_ahead, _R.device_valid

    def __init__(self, state, dev, backend):
        (self.host_stale, self.host_touched), self.dev_state, self.backend = state, dev, backend


class _FakeBackend(pde_hip.spectrum.SpectrumMixin):
    stream = None

    def __init__(self, entries=("fft_supported", "shell_spectrum"), refuse=False):
        self._lib, self.device_calls = _FakeLib(entries, refuse), 0

    def _device_shells(self, dev, edges):
        self.device_calls += 1
        return pde_hip.spectrum.host_shells(dev.data, 0, dev.info.dx, edges)


class _FakeField:
    def __init__(self, data, link=None):
        self.grid, self.data = pde_hip.UnitGrid([8, 16], periodic=True), data
        if link is not None:
            self.__dict__["_hip_link"] = link


@pytest.mark.parametrize("state, ahead", (((False, True), False), ((False, False), False), ((True, False), True)), ids=("host_current", "equal", "device_ahead"))
def test_residency_rules_with_stand_ins(state, ahead):
    """The device answers only while its copy is AHEAD, the kernels take the array, the entry points are there and the dry run agrees."""
    data = np.random.default_rng(1).normal(size=(8, 16))
    for kwargs, complex_pairs, takes in (({}, False, True), ({"refuse": True}, False, False), ({"entries": ("fft_supported",)}, False, False),
                                         ({"entries": ()}, False, False), ({}, True, False)):
        backend = _FakeBackend(**kwargs)
        field = _FakeField(data)
        field.__dict__["_hip_link"] = _FakeLink(state, _FakeArray(data, complex_pairs), backend)
        got = backend.make_spectrum()(field)
        assert got.on_device == (ahead and takes) and backend.device_calls == int(ahead and takes)
        assert int(got.counts.sum()) == data.size
    backend = _FakeBackend()
    assert not backend.make_spectrum()(_FakeField(data)).on_device and backend.device_calls == 0          # a field without a link


def _run(seen, t_range=2.0):
    grid = pde_hip.UnitGrid([16, 32], periodic=True)
    state = pde_hip.ScalarField(grid, 1.0 + K.cosine_field((16, 32), ((1, (2, 0)), (2, (0, 5)))))

    def callback(field, t):
        link = field.__dict__.get("_hip_link")
        resident = link is not None and link.host_stale
        before = link.downloads if link is not None else None
        got = pde_hip.field_spectrum(field)
        seen.append({"resident": resident, "on_device": got.on_device, "before": before, "after": link.downloads if link is not None else None,
                     "got": got, "side": link.dev_state.get_valid() if resident else np.array(field.data)})

    return pde_hip.DiffusionPDE(0.5).solve(state, t_range=t_range, dt=0.05, solver="euler", backend=pde_hip.get_backend("hip"), tracker=callback,
                                           interval=0.5)


def _check_seen(seen):
    for s in seen:
        side, got = s["side"], s["got"]
        assert int(got.counts.sum()) == side.size
        assert abs(got.total - np.mean(side * side)) <= 1e-12 * np.mean(side * side)
        assert got.k_peak == 5.0 / 32.0


def test_a_callback_leaves_the_state_on_the_device():
    seen = []
    with spectrum_shimlib.use_shim():
        res = _run(seen)
        link = res.__dict__["_hip_link"]
        resident = [s for s in seen if s["resident"]]
        assert len(resident) >= 3 and all(s["on_device"] and s["before"] == s["after"] == 0 for s in resident), seen
        assert link.downloads == 0
        _check_seen(seen)
        res.data                                             # noqa: B018  (the download)
        uploads = link.uploads
        late = pde_hip.field_spectrum(res)
        assert not late.on_device and link.uploads == uploads          # host-current: the host path, nothing uploaded


def test_a_library_without_the_entry_points_takes_the_host_path():
    seen = []
    with stats_shimlib.use_shim():
        _run(seen, 1.0)
    assert seen and not any(s["on_device"] for s in seen)
    _check_seen(seen)


def test_complex_data_take_the_host_path(shim):
    backend = pde_hip.get_backend("hip")
    grid = pde_hip.UnitGrid([8, 16], periodic=True)
    rng = np.random.default_rng(8)
    data = rng.normal(size=(8, 16)) + 1j * rng.normal(size=(8, 16))
    got = backend.make_spectrum(grid)(data)
    assert not got.on_device and int(got.counts.sum()) == data.size
    assert abs(got.total - np.mean(np.abs(data) ** 2)) <= 1e-12 * np.mean(np.abs(data) ** 2)
