"""GPU: the step-0 kernel (csrc/ingest.hip) against NumPy, bit for bit, through both entry points:
``origin_cube_ingest_planes`` on bytes uploaded by the test and ``origin_cube_read`` on a file.

Expected values, computed in float32 as the kernel defines them:
    d, s = DATA, STAT as float32;  m = ~isfinite(d) | ~isfinite(s)
    raw = where(m, 0, d);  var = where(m, inf, s);  mask = m
    sum = np.add.reduce(raw.astype(float64), axis=0)   (plane by plane);  cnt = (~m).sum(0)
compared through the uint32 / uint8 / uint64 views: -0.0, denormals and the sign of a zero sum
count.  Shapes cover S % 4 == 0 (16-byte form) and != 0 (scalar form), S below one wave and several
blocks; one large plane (1500 x 1500 > 256 CUs x 32 blocks x 64 lanes x 4 voxels) runs the grid-stride
loop a second time."""
import numpy as np
import pytest

from origin_amd import _capi, fitsio
from origin_amd.device import DeviceArray, default_context

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (4, 8), (7, 9), (24, 28), (33, 64)]
NZS = [1, 2, 7, 45]
PAIRS = [(-32, -32), (-32, -64), (-64, -32), (-64, -64)]
DENORMAL = float(np.float32(1e-41))
LONG_HEADER = {f"HIERK{i:02d}": float(i) for i in range(80)}     # a primary header of 3 blocks


def chunkings(Nz):
    return sorted({0, 1, 3, Nz, Nz + 5})


def make_case(Nz, Ny, Nx, bd, bs, seed=0):
    """(data, stat) as float64 arrays whose values are float32 numbers -- except, in a BITPIX -64
    unit, 1e39 (inf as float32: masked) and 1e-50 (0 as float32: kept) -- with every special
    value of the contract scattered over the voxels, one spaxel masked at every z and one plane
    masked at every spaxel."""
    rng = np.random.default_rng(seed + 1000 * Nz + Ny * Nx)
    n = Nz * Ny * Nx
    data = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    stat = (rng.random(n) + 0.5).astype(np.float32).astype(np.float64)
    nan, inf = np.nan, np.inf
    specials = [(nan, None), (inf, None), (-inf, None), (None, nan), (None, inf), (None, -inf),
                (nan, nan), (inf, -inf), (-0.0, None), (DENORMAL, None), (-DENORMAL, DENORMAL),
                (None, 0.0), (None, -1.5), (0.0, -0.0)]
    if bd == -64:
        specials += [(1e39, None), (-1e39, None), (1e-50, None)]
    if bs == -64:
        specials += [(None, 1e39), (None, 1e-50)]
    at = rng.permutation(n)
    for k, (d, s) in enumerate(specials * 2):
        i = at[k % n]
        if d is not None:
            data[i] = d
        if s is not None:
            stat[i] = s
    data, stat = data.reshape(Nz, Ny, Nx), stat.reshape(Nz, Ny, Nx)
    if Ny * Nx > 1:
        data[:, Ny // 2, Nx - 1] = nan                       # a spaxel masked at every z
        data[:, 0, 0] = -0.0                                 # a spaxel that holds only -0.0
        stat[:, 0, 0] = 1.0
    if Nz > 2:
        stat[Nz // 2] = nan                                  # a plane masked at every spaxel
    return data, stat


def expected(data, stat):
    with np.errstate(over="ignore"):
        d, s = data.astype(np.float32), stat.astype(np.float32)
    m = ~np.isfinite(d) | ~np.isfinite(s)
    raw = np.where(m, np.float32(0), d)
    var = np.where(m, np.float32(np.inf), s)
    wsum = np.add.reduce(raw.astype(np.float64), axis=0)
    return raw, var, m.astype(np.uint8), wsum, (~m).sum(0).astype(np.int32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, want, what):
    for name, g, w in zip(("raw", "var", "mask", "sum", "cnt"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        bad = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5]}: " \
                              f"{g.ravel()[bad[:5]]} != {w.ravel()[bad[:5]]}"


class Outputs:
    def __init__(self, ctx, shape):
        Nz, Ny, Nx = shape
        self.ctx, self.Nz, self.S = ctx, Nz, Ny * Nx
        self.raw, self.var = DeviceArray(ctx, shape, np.float32), DeviceArray(ctx, shape, np.float32)
        self.mask = DeviceArray(ctx, shape, np.uint8)
        self.wsum, self.wcnt = DeviceArray(ctx, (Ny, Nx), np.float64), DeviceArray(ctx, (Ny, Nx), np.int32)
        for a in (self.raw, self.var, self.mask, self.wsum, self.wcnt):
            a.fill_bytes(0x5a)        # whatever is not written shows

    def host(self):
        return tuple(a.to_host() for a in (self.raw, self.var, self.mask, self.wsum, self.wcnt))


def byte_route(ctx, data, stat, bd, bs, ppc):
    """The planes uploaded as file bytes, ``ppc`` at a time, and ingested chunk after chunk."""
    out = Outputs(ctx, data.shape)
    Nz, S = out.Nz, out.S
    db = np.ascontiguousarray(data, ">f4" if bd == -32 else ">f8").view(np.uint8).reshape(Nz, -1)
    sb = np.ascontiguousarray(stat, ">f4" if bs == -32 else ">f8").view(np.uint8).reshape(Nz, -1)
    out.wsum.fill_bytes(0)
    out.wcnt.fill_bytes(0)
    keep = []
    for z0 in range(0, Nz, ppc):
        z1 = min(Nz, z0 + ppc)
        d, s = ctx.to_device(db[z0:z1]), ctx.to_device(sb[z0:z1])
        keep += [d, s]
        _capi.call("origin_cube_ingest_planes", ctx.handle, d.p, bd, s.p, bs, z1 - z0, S,
                   out.raw.view(z0 * S, (S,)).p, out.var.view(z0 * S, (S,)).p,
                   out.mask.view(z0 * S, (S,)).p, out.wsum.p, out.wcnt.p)
    ctx.sync()
    return out.host()


def file_route(ctx, path, ppc):
    info = fitsio.open_cube(path)
    out = Outputs(ctx, info.shape)
    with open(path, "rb", buffering=0) as f:
        _capi.call("origin_cube_read", ctx.handle, f.fileno(), info.off_data, info.bitpix_data,
                   info.off_stat, info.bitpix_stat, out.Nz, out.S, ppc, out.raw.p, out.var.p,
                   out.mask.p, out.wsum.p, out.wcnt.p)
    return out.host()


@pytest.fixture(scope="module")
def ctx():
    return default_context(0)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d_%d" % p)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ingest_matches_numpy(ctx, tmp_path, shape, pair):
    """Every Nz and chunking of one plane shape and BITPIX pair, through both routes; the file
    has a three-block primary header and STAT before DATA for every other Nz."""
    bd, bs = pair
    for k, Nz in enumerate(NZS):
        data, stat = make_case(Nz, *shape, bd, bs)
        want = expected(data, stat)
        path = fitsio.write_cube(str(tmp_path / f"c{Nz}.fits"), data, stat, bitpix=pair,
                                 primary_header=LONG_HEADER if k % 2 else None,
                                 stat_first=bool(k % 2))
        for ppc in chunkings(Nz):
            what = f"Nz={Nz} planes_per_chunk={ppc}"
            assert_same(file_route(ctx, path, ppc), want, "file " + what)
            if ppc:
                assert_same(byte_route(ctx, data, stat, bd, bs, ppc), want, "bytes " + what)


def test_contents_reach_every_special_value():
    """The generator does put each special value where it stays visible (at the largest shape)."""
    data, stat = make_case(45, 33, 64, -64, -64)
    raw, var, m, wsum, cnt = expected(data, stat)
    keep = m == 0
    assert np.isnan(data).any() and np.isposinf(data).any() and np.isneginf(data).any()
    assert np.isnan(stat).any() and np.isposinf(stat).any() and np.isneginf(stat).any()
    assert (np.signbit(raw) & (raw == 0) & keep).any()                        # -0.0 kept
    assert ((raw != 0) & (np.abs(raw) < np.finfo(np.float32).tiny) & keep).any()   # denormal kept
    assert ((var == 0) & keep).any() and ((var < 0) & keep).any()
    assert (m[(np.abs(data) == 1e39)] == 1).all() and (np.abs(data) == 1e39).any()
    assert ((data == 1e-50) & keep & (raw == 0)).any()
    assert (cnt == 0).any() and (m.all(axis=(1, 2))).any()
    # NumPy reduces from the identity +0.0: a spaxel of nothing but -0.0 sums to +0.0
    assert (data[:, 0, 0] == 0).all() and np.signbit(data[:, 0, 0]).all()
    assert wsum[0, 0] == 0 and not np.signbit(wsum[0, 0])


def test_unaligned_file_equals_bytes(ctx, tmp_path):
    """Data units at offsets that are no multiple of a 4096-byte page (a primary header of three
    blocks, STAT first, odd plane sizes): the file route gives what the byte route gives."""
    for pair in PAIRS:
        data, stat = make_case(7, 7, 9, *pair, seed=3)
        path = fitsio.write_cube(str(tmp_path / "u.fits"), data, stat, bitpix=pair,
                                 primary_header=LONG_HEADER, stat_first=True)
        info = fitsio.open_cube(path)
        assert info.off_stat < info.off_data and info.off_data % 4096 and info.off_stat % 4096
        assert_same(file_route(ctx, path, 3), byte_route(ctx, data, stat, *pair, 3), str(pair))


def test_grid_stride_on_a_large_plane(ctx, tmp_path):
    rng = np.random.default_rng(5)
    shape = (2, 1500, 1500)
    data = rng.standard_normal(shape).astype(np.float32).astype(np.float64)
    stat = (rng.random(shape) + 0.5).astype(np.float32).astype(np.float64)
    data[rng.random(shape) < 0.01] = np.nan
    stat[1, -1, -1] = np.inf
    path = fitsio.write_cube(str(tmp_path / "big.fits"), data, stat, bitpix=-32)
    assert_same(file_route(ctx, path, 0), expected(data, stat), "1500 x 1500")


def test_read_cube_white_image(ctx, tmp_path):
    data, stat = make_case(7, 24, 28, -64, -32)
    raw, var, m, wsum, cnt = expected(data, stat)
    hdr = {"CRVAL1": 53.0, "CRVAL3": 4750.0}
    path = fitsio.write_cube(str(tmp_path / "w.fits"), data, stat, bitpix=(-64, -32), header=hdr)
    d_raw, d_var, d_mask, white, wcs, wave = fitsio.read_cube(path, ctx, planes_per_chunk=2)
    assert (d_raw.dtype, d_var.dtype, d_mask.dtype) == (np.float32, np.float32, np.uint8)
    assert_same((d_raw.to_host(), d_var.to_host(), d_mask.to_host()), (raw, var, m), "read_cube")
    assert white.dtype == np.float64 and (cnt == 0).any()
    assert np.array_equal(np.isnan(white), cnt == 0)
    assert np.array_equal(white[cnt > 0], wsum[cnt > 0] / cnt[cnt > 0])
    assert dict(wcs) == {"CRVAL1": 53.0} and dict(wave) == {"CRVAL3": 4750.0}


def test_short_file_is_an_error(ctx, tmp_path):
    """A file that shrinks between open_cube and the read: ORIGIN_E_STATE, not a hang."""
    data, stat = make_case(7, 7, 9, -32, -32)
    path = fitsio.write_cube(str(tmp_path / "s.fits"), data, stat)
    info = fitsio.open_cube(path)
    out = Outputs(ctx, info.shape)
    with open(path, "rb", buffering=0) as f:
        with pytest.raises(_capi.OriginHipError) as e:
            _capi.call("origin_cube_read", ctx.handle, f.fileno(), info.off_data, -32,
                       info.off_stat + 4 * 2880, -32, out.Nz, out.S, 2, out.raw.p, out.var.p,
                       out.mask.p, out.wsum.p, out.wcnt.p)
    assert e.value.code == -5
