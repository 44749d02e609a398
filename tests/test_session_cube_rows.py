"""GPU: ``SimpleOrig.from_cube(..., devices=[...])`` -- every rank of the tiled session reads the
rows of its own band from the cube file (``TiledSession.open_cube``, ``origin_cube_read_rows``) and
step 1 runs on the bands where they are -- against the tiled session made from the arrays NumPy
derives from the same data.  The reader leaves bitwise those arrays (tests/test_hip_cube_rows.py),
so every output of steps 1-6 has to be *equal*; and between ``from_cube`` and the end of step 1 no
transfer, in either direction, may carry a whole cube."""
import logging
import threading

import numpy as np
import pytest

from origin_amd import _capi, fitsio, session, synth
from origin_amd.device import Context, DeviceArray
from origin_amd.steps import LazyCube, SimpleOrig
from test_session_from_cube import WAVE, WCS, assert_equal_sessions, chain

pytestmark = pytest.mark.gpu

# the field of tests/test_session_from_cube.py for two ranks; 50 rows for three (17 + 16 + 17)
FIELDS = {2: (160, 48, 52), 3: (160, 50, 52)}


class Case:
    pass


def make_case(tmp, shape):
    c = Case()
    Nz, Ny, Nx = shape
    c.f, raw, var, mask = synth.small_case(Nz=Nz, Ny=Ny, Nx=Nx, area_size=24, masked_border=2)
    rng = np.random.default_rng(11)
    data, stat = raw.astype(np.float64), var.astype(np.float64)
    data[mask] = np.nan
    stat[mask] = np.nan

    def interior(n):
        return (rng.integers(0, Nz, n), rng.integers(4, Ny - 4, n), rng.integers(4, Nx - 4, n))
    data[interior(12)] = np.nan
    stat[interior(4)] = np.nan
    m = ~np.isfinite(data) | ~np.isfinite(stat)
    c.data, c.stat, c.mask = data, stat, m
    c.raw = np.where(m, 0, data).astype(np.float32)
    c.var = np.where(m, np.inf, stat).astype(np.float32)
    c.psf = c.f.PSF.astype(float)
    c.path = fitsio.write_cube(str(tmp / "cube.fits"), data, stat, header={**WCS, **WAVE})
    return c


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(world):
        if world not in made:
            made[world] = make_case(tmp_path_factory.mktemp(f"cube{world}"), FIELDS[world])
        return made[world]
    return get


class Spy:
    """Names of the library calls, and the element counts of everything that crosses between the
    host and a device: ``DeviceArray.to_host*``, ``Context.to_device``, and the gathers of a
    ``TiledCube`` (which are band-sized transfers each, and a whole cube together)."""

    def __init__(self, monkeypatch):
        self.calls, self.moves, self.on = [], [], True
        lock = threading.Lock()
        call = _capi.call

        def spy_call(name, *a):
            with lock:
                self.calls.append(name)
            return call(name, *a)
        monkeypatch.setattr(_capi, "call", spy_call)

        def wrap(cls, name, size):
            fn = getattr(cls, name)

            def spied(obj, *a, **k):
                if self.on:
                    with lock:
                        self.moves.append((f"{cls.__name__}.{name}", int(size(obj, *a))))
                return fn(obj, *a, **k)
            monkeypatch.setattr(cls, name, spied)
        for cls in (DeviceArray, session.TiledCube):
            wrap(cls, "to_host", lambda obj, *a: obj.size)
            wrap(cls, "to_host_f64", lambda obj, *a: obj.size)
        wrap(Context, "to_device", lambda obj, host, *a: np.size(host))


@pytest.mark.parametrize("world", [2, 3])
def test_tiled_from_cube_equals_the_array_session(cases, monkeypatch, world):
    c = cases(world)
    f, devices = c.f, [0] * world
    Nz, Ny, Nx = FIELDS[world]
    spy = Spy(monkeypatch)
    one = SimpleOrig.from_cube(c.path, f.profiles, c.psf, FWHM_PSF=3.3, devices=devices)
    sess = one._hip_session
    assert sess.world == world and one.shape == (Nz, Ny, Nx)
    for cube, dtype in ((one.cube_raw, np.float64), (one.var, np.float64), (one.mask, bool)):
        assert isinstance(cube, LazyCube) and isinstance(cube.dev, session.TiledCube)
        assert cube._dtype == dtype and cube._host is None and cube.dev.group is sess.group
    rows = [sess.p1.tile(r).y1 - sess.p1.tile(r).y0 for r in range(world)]
    assert sum(rows) == Ny and (world == 2 or len(set(rows)) > 1)       # three ranks: uneven bands
    for r in range(world):
        assert sess.rk[r]["raw"].shape == (Nz, rows[r], Nx)
    one.step01_preprocessing()
    spy.on = False
    # every rank read its band from the file, nobody the whole field
    assert spy.calls.count("origin_cube_read_rows") == world
    assert spy.calls.count("origin_cube_read") == 0
    whole = [m for m in spy.moves if m[1] >= Nz * Ny * Nx]
    assert not whole, whole
    assert spy.moves                                                     # (the spy does see transfers)
    assert one.cube_raw._host is None and one.var._host is None and one.mask._host is None
    assert sess.host_mask is None
    # step 1 ran on the arrays the file read left
    for r in range(world):
        assert one.cube_raw.dev.parts[r][0] is sess.rk[r]["raw"]

    chain_rest(one, f.areamap)
    two = chain(SimpleOrig(c.raw, c.var, c.mask, c.psf, f.profiles, devices=devices), f.areamap)
    assert_equal_sessions(one, two)

    # the one-device session from the same file: white image and, on demand, the host cubes
    solo = SimpleOrig.from_cube(c.path, f.profiles, c.psf, FWHM_PSF=3.3)
    assert one.ima_white.dtype == np.float64 and one.ima_white.shape == (Ny, Nx)
    assert np.isnan(solo.ima_white).any()
    assert np.array_equal(one.ima_white.view(np.uint64), solo.ima_white.view(np.uint64))
    for name, dtype in (("cube_raw", np.float64), ("var", np.float64), ("mask", bool)):
        a, b = getattr(one, name)._data, getattr(solo, name)._data
        assert a.dtype == b.dtype == dtype and np.array_equal(a, b), name
    assert np.array_equal(one.cube_raw._data, c.raw) and np.array_equal(one.mask._data, c.mask)
    assert dict(one.wcs_header) == WCS and dict(one.wave_header) == WAVE
    one._hip_session.close()
    two._hip_session.close()


def chain_rest(orig, areamap):
    orig.step02_areas.set_areamap(areamap)
    orig.step03_compute_PCA_threshold()
    orig.step04_compute_greedy_PCA()
    orig.step05_compute_TGLR()
    orig.step06_compute_purity_threshold(purity=0.8)


def test_the_spy_sees_a_host_round_trip(cases, monkeypatch):
    """What the transfer check is there for: a tiled session given ``LazyCube``s over whole-field
    device arrays (the route ``from_cube`` took before) does move whole cubes."""
    c = cases(2)
    Nz, Ny, Nx = FIELDS[2]
    raw, var, mask = fitsio.read_cube(c.path)[:3]
    spy = Spy(monkeypatch)
    orig = SimpleOrig(LazyCube(raw), LazyCube(var), LazyCube(mask, dtype=bool), c.psf, c.f.profiles,
                      devices=[0, 0])
    orig.step01_preprocessing()
    assert len([m for m in spy.moves if m[1] >= Nz * Ny * Nx]) >= 2
    orig._hip_session.close()


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one", "two"])
def test_dq_option(cases, tmp_path, caplog, devices):
    c = cases(2)
    Nz, Ny, Nx = FIELDS[2]
    voxels = [(3, 10, 20), (Nz - 1, Ny - 6, 7)]          # one in each band of two ranks
    dq = np.zeros(c.data.shape, np.int16)
    for v in voxels:
        assert not c.mask[v]
        dq[v] = 0x100
    path = fitsio.write_cube(str(tmp_path / "dq.fits"), c.data, c.stat, dq=dq, dq_bitpix=16)
    kw = dict(FWHM_PSF=3.3, devices=devices)
    with caplog.at_level(logging.WARNING, logger="origin_amd.fitsio"):
        flagged = SimpleOrig.from_cube(path, c.f.profiles, c.psf, dq=True, **kw)
        assert not [r for r in caplog.records if "DQ" in r.getMessage()]
        plain = SimpleOrig.from_cube(path, c.f.profiles, c.psf, **kw)
        assert [r for r in caplog.records if "ignored" in r.getMessage()]
    want = c.mask.copy()
    assert np.array_equal(plain.mask._data, want)
    assert np.array_equal(plain.cube_raw._data, c.raw)
    for v in voxels:
        want[v] = True
    assert np.array_equal(flagged.mask._data, want)
    for v in voxels:
        assert flagged.cube_raw._data[v] == 0 and flagged.var._data[v] == np.inf
        assert plain.cube_raw._data[v] == c.raw[v] != 0
    rest = ~want
    assert np.array_equal(flagged.cube_raw._data[rest], c.raw[rest])
    # the white image loses the flagged voxels
    with np.errstate(invalid="ignore"):
        white = np.where(want, 0, c.raw).astype(np.float64).sum(0) / (~want).sum(0)
    assert np.allclose(flagged.ima_white, white, rtol=1e-12, atol=0, equal_nan=True)
    assert flagged.ima_white[voxels[0][1:]] != plain.ima_white[voxels[0][1:]]
    for o in (flagged, plain):
        if devices:
            o._hip_session.close()
